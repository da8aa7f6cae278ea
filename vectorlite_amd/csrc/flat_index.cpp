// flat_index.cpp -- host logic of the GPU flat index (see flat_index.hpp).
//
// Mirrors `impl VectorIndex for FlatIndex` (reference src/index/flat.rs:82-135): same argument
// meaning, same error behaviour, same result order.  All arithmetic on vectors runs in the HIP
// kernels (kernels.hip); the host only stages queries, keeps the position -> id table and maps
// positions back to ids for the k winners (the reference re-attaches text/metadata the same way,
// src/index/flat.rs:106-114).  There is no CPU compute fallback.
#include "flat_index.hpp"
#include "delete_plan.hpp"
#include "update_plan.hpp"
#include "lazy_buffers.hpp"
#include "shard.hpp"
#include "score_bound.hpp"
#include "subset_batch_plan.hpp"
#include "masked_batch_plan.hpp"
#include "where_plan.hpp"
#include "grouped_batch_plan.hpp"
#include "mmr_batch_plan.hpp"

#include <chrono>

#include <algorithm>
#include <limits>
#include <map>
#include <type_traits>
#include <cmath>
#include <cstring>

namespace vl {

// ---------------------------------------------------------------------------------------------
// thread-local diagnostics
// ---------------------------------------------------------------------------------------------
namespace {
thread_local std::string t_last_error;
thread_local uint64_t t_dim_expected = 0, t_dim_actual = 0;
thread_local int t_last_path = PATH_NONE;
}  // namespace

void set_last_error(const std::string& msg) { t_last_error = msg; }
const char* last_error() { return t_last_error.c_str(); }
void set_dim_mismatch(uint64_t expected, uint64_t actual)
{
    t_dim_expected = expected;
    t_dim_actual = actual;
}
void get_dim_mismatch(uint64_t* expected, uint64_t* actual)
{
    if (expected) *expected = t_dim_expected;
    if (actual) *actual = t_dim_actual;
}
void set_last_path(int p) { t_last_path = p; }
int last_path() { return t_last_path; }

#define VL_HIP(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            set_last_error(std::string(#expr) + ": " + hipGetErrorString(e_));                   \
            (void)hipGetLastError(); /* a failed call (hipMalloc out of memory ...) leaves the thread's sticky error behind: the next launch's hipGetLastError() must not report it */ \
            return (e_ == hipErrorOutOfMemory) ? (int)ERR_OOM : (int)ERR_DEVICE;                 \
        }                                                                                        \
    } while (0)

// the argument checks of a diversified search that need no handle and no device (c_api.cpp runs them first)
int mmr_check_args(uint64_t k, uint64_t fetch_k, double lambda)
{
    if (!(lambda >= 0.0 && lambda <= 1.0)) {
        set_last_error("lambda must lie in [0, 1]");
        return ERR_INVALID_ARG;
    }
    if (fetch_k < k) {
        set_last_error("fetch_k must be at least k");
        return ERR_INVALID_ARG;
    }
    if (fetch_k > (uint64_t)MMR_MAX_FETCH) {
        set_last_error("fetch_k exceeds VL_MMR_MAX_FETCH (" + std::to_string(MMR_MAX_FETCH) + ")");
        return ERR_INVALID_ARG;
    }
    return OK;
}

#define VL_TRY(expr)              \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != OK) return rc_; \
    } while (0)

namespace {
constexpr double DOMAIN_MAX_ABS = 1099511627776.0;          // 2^40
constexpr double DOMAIN_MIN_NORM = 9.094947017729282e-13;   // 2^-40
constexpr size_t BOUNCE_BYTES = 64ull << 20;

template <typename T>
int dev_alloc(T** p, size_t count)
{
    *p = nullptr;
    if (count == 0) return OK;
    VL_HIP(hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
    return OK;
}
template <typename T>
int pinned_alloc(T** p, size_t count)
{
    *p = nullptr;
    VL_HIP(hipHostMalloc(reinterpret_cast<void**>(p), count * sizeof(T), hipHostMallocDefault));
    return OK;
}
// what lazy_buffers.hpp allocates with here: device memory, or pinned host memory
struct HipMem {
    int alloc(void** p, size_t bytes, bool pinned) const
    {
        unsigned char** b = reinterpret_cast<unsigned char**>(p);
        return pinned ? pinned_alloc(b, bytes) : dev_alloc(b, bytes);
    }
    void release(void* p, bool pinned) const { (void)(pinned ? hipHostFree(p) : hipFree(p)); }
};

// ---- lazily made workspace buffers (all or nothing: a failed call leaves the workspace as it found it) ----
int ensure_scores(Workspace* ws, uint64_t rows)  // the exact scans' score of every row
{
    return grow(HipMem{}, ws->scores_cap, std::max<size_t>(rows, 1024), {dev_buf(ws->d_scores, std::max<size_t>(rows, 1024))});
}
int ensure_out(Workspace* ws, uint64_t need)  // ranked (position, score) pairs on the device: the sort's, the range routes'
{
    return grow(HipMem{}, ws->out_cap, need, {dev_buf(ws->d_out_pos, need), dev_buf(ws->d_out_scores, need)});
}
int ensure_range_ws(Workspace* ws, uint64_t sort_cap, uint64_t out_cap)
{
    VL_TRY(ensure_set(HipMem{}, {dev_buf(ws->rg_ctr, RANGE_CTR_WORDS), pinned_buf(ws->rg_h_ctr, RANGE_CTR_WORDS),
                                 pinned_buf(ws->rg_h_pos, RANGE_SMALL), pinned_buf(ws->rg_h_scores, RANGE_SMALL)}));
    VL_TRY(grow(HipMem{}, ws->rg_sort_cap, sort_cap, {dev_buf(ws->rg_keys, sort_cap), dev_buf(ws->rg_pv, sort_cap)}));
    return ensure_out(ws, out_cap);
}
int ensure_range_candidates(Workspace* ws)  // the fast range scan's candidate positions and their scores
{
    return ensure_set(HipMem{}, {dev_buf(ws->rg_cand, RANGE_CAND_MAX), dev_buf(ws->rg_scores, RANGE_CAND_MAX)});
}
int ensure_group_ws(Workspace* ws, uint64_t n_groups)
{
    VL_TRY(ensure_set(HipMem{}, {dev_buf(ws->gp_ctr, RANGE_CTR_WORDS + 1), dev_buf(ws->gp_lists, (size_t)GROUP_TOP_LISTS * KP),
                                 dev_buf(ws->gp_cand, KP), dev_buf(ws->gp_scores, KP), dev_buf(ws->gp_out_keys, GROUPED_MAX_K),
                                 pinned_buf(ws->gp_h_ctr, RANGE_CTR_WORDS + 1), pinned_buf(ws->gp_h_scores, KP),
                                 pinned_buf(ws->gp_h_keys, GROUPED_MAX_K)}));
    return grow(HipMem{}, ws->gp_cap, n_groups, {dev_buf(ws->gp_best, n_groups), dev_buf(ws->gp_first, n_groups)});
}

// ---- the single-query protocol's small steps ----
// the next result stamp of this workspace (never 0), the pinned block's stamp cleared for it
uint32_t next_stamp(Workspace* ws)
{
    uint32_t seq = ++ws->seq;
    if (seq == 0) seq = ++ws->seq;
    ws->h_result->seq = 0;
    return seq;
}
// the f32 query a scan takes in its kernel arguments: `width` floats, zero past dim (nearest even, like load_q4 on the device)
const float* stage_q32(Workspace* ws, const double* query, uint64_t dim, uint32_t width)
{
    if (ws->q32.size() < width) ws->q32.assign(width, 0.0f);
    for (uint64_t i = 0; i < dim; ++i) ws->q32[i] = (float)query[i];
    return ws->q32.data();
}

// The answer's positions -> the caller's arrays, entry i from pos_at(i) / score_at(i); `what` names the route.
template <typename PosAt, typename ScoreAt>
int deliver(const char* what, const std::vector<uint64_t>& row_ids, uint64_t count, PosAt pos_at, ScoreAt score_at, uint64_t* out_pos,
            uint64_t* out_ids, double* out_scores)
{
    const uint64_t n = row_ids.size();
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t p = pos_at(i);
        if (p >= n) {
            set_last_error(std::string(what) + " returned an out-of-range position (kernel bug)");
            return ERR_DEVICE;
        }
        if (out_pos) out_pos[i] = p;
        if (out_ids) out_ids[i] = row_ids[p];
        out_scores[i] = score_at(i);
    }
    return OK;
}
int deliver(const char* what, const std::vector<uint64_t>& row_ids, const uint32_t* pos, const double* scores, uint64_t count,
            uint64_t* out_pos, uint64_t* out_ids, double* out_scores)
{
    return deliver(what, row_ids, count, [&](uint64_t i) { return pos[i]; }, [&](uint64_t i) { return scores[i]; }, out_pos, out_ids,
                   out_scores);
}
// ... from result blocks: entry i is blocks[i / KP]'s (i % KP)-th
int deliver(const char* what, const std::vector<uint64_t>& row_ids, const SearchResultBlock* blocks, uint64_t count, uint64_t* out_pos,
            uint64_t* out_ids, double* out_scores)
{
    return deliver(what, row_ids, count, [&](uint64_t i) { return blocks[i / KP].pos[i % KP]; },
                   [&](uint64_t i) { return blocks[i / KP].score[i % KP]; }, out_pos, out_ids, out_scores);
}

// Token tables (filters, group tables).  token_find: the entry of `token`.  token_take: the same, removed from the table;
// the caller's reference frees it outside the lock, and only once no search uses it.
template <typename Map>
int token_find(std::mutex& mu, const Map& table, uint64_t token, const char* unknown, typename Map::mapped_type* out)
{
    std::lock_guard<std::mutex> g(mu);
    auto it = table.find(token);
    if (it == table.end()) {
        set_last_error(unknown);
        return ERR_INVALID_ARG;
    }
    *out = it->second;
    return OK;
}
template <typename Map>
int token_take(std::mutex& mu, Map& table, uint64_t token, const char* unknown, typename Map::mapped_type* out)
{
    std::lock_guard<std::mutex> g(mu);
    auto it = table.find(token);
    if (it == table.end()) {
        set_last_error(unknown);
        return ERR_INVALID_ARG;
    }
    *out = std::move(it->second);
    table.erase(it);
    return OK;
}
constexpr const char* UNKNOWN_FILTER = "unknown or destroyed filter";
constexpr const char* UNKNOWN_GROUPS = "unknown or destroyed group table";
constexpr const char* UNKNOWN_ATTR = "unknown or destroyed attribute column";
}  // namespace

Workspace::~Workspace()
{
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    void* dev[] = {d_q64, d_partials, d_partials64, d_result, d_nan, d_scores, d_okeys,
                   d_opos, d_out_pos, d_out_scores, d_positions, d_dists, rg_ctr, rg_cand, rg_scores, rg_keys, rg_pv, mmr_sim,
                   rb_ctr, rb_min, rb_sv_score, rb_sv_pos, gp_best, gp_first, gp_lists, gp_cand, gp_scores, gp_ctr, gp_out_keys,
                   gb_keep, gb_m, mb_ranked};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    void* host[] = {h_q64, h_result, h_nan, mf_h_q64, mf_h_result, mf_h_dom, k3_h_q64, k3_h_result, rg_h_ctr, rg_h_pos, rg_h_scores,
                    rb_h_thr, rb_h_min, rb_h_ctr, rb_h_cnt, rb_h_pos, rb_h_scores, gp_h_ctr, gp_h_scores, gp_h_keys,
                    gb_h_result};
    for (void* p : host)
        if (p) (void)hipHostFree(p);
    void* mfd[] = {mf.q_bf16, mf.gmax, mf.thr, mf.cand, mf.cnt, mf_d_q64, mf_lists, mf_scores, k3_d_q64};
    for (void* p : mfd)
        if (p) (void)hipFree(p);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (hipEvent_t e : mf_ev_done)
        if (e) (void)hipEventDestroy(e);
    if (mf_ev_h2d) (void)hipEventDestroy(mf_ev_h2d);
    if (stream) (void)hipStreamDestroy(stream);
}

// ---------------------------------------------------------------------------------------------
// lifecycle
// ---------------------------------------------------------------------------------------------
GpuFlatIndex::GpuFlatIndex(uint64_t dim, int device)
    : dim_(dim), ld_((uint32_t)((dim + 3) & ~3ull)), device_(device)
{
    ws_pool_ = attach_pool(device, dim);
}

namespace {
// Copies a query into its staging slot and decides whether it lies in the fast-path domain (finite, |v| <= 2^40,
// norm 0 or >= 2^-40).  The norm only feeds the error bound and that domain test (the kernels recompute every score
// from the values), so it is summed with four partial accumulators the compiler can vectorise; a query outside the
// domain is staged as zeros (keeps the f32 / bf16 scans finite) with norm 0 and answered on the exact path.
bool stage_query(const double* q, double* dst, uint64_t dim, double* norm_out)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
    uint64_t i = 0;
    for (; i + 4 <= dim; i += 4) {
        const double a = q[i], b = q[i + 1], c = q[i + 2], d = q[i + 3];
        dst[i] = a;
        dst[i + 1] = b;
        dst[i + 2] = c;
        dst[i + 3] = d;
        s0 += a * a;
        s1 += b * b;
        s2 += c * c;
        s3 += d * d;
        const double fa = std::fabs(a), fb = std::fabs(b), fc = std::fabs(c), fd = std::fabs(d);
        m0 = fa > m0 ? fa : m0;
        m1 = fb > m1 ? fb : m1;
        m2 = fc > m2 ? fc : m2;
        m3 = fd > m3 ? fd : m3;
    }
    for (; i < dim; ++i) {
        const double a = q[i];
        dst[i] = a;
        s0 += a * a;
        const double fa = std::fabs(a);
        m0 = fa > m0 ? fa : m0;
    }
    const double qq = (s0 + s1) + (s2 + s3);
    const double m01 = m0 > m1 ? m0 : m1, m23 = m2 > m3 ? m2 : m3;
    const double qmax = m01 > m23 ? m01 : m23;
    const double norm = std::sqrt(qq);
    // a NaN component makes qq NaN (the max ignores it); an infinity shows up in qmax (and qq)
    const bool finite = qq == qq && qmax <= 1.797693134862315708e308 && norm <= 1.797693134862315708e308;
    const bool in_domain = finite && qmax <= DOMAIN_MAX_ABS && (norm == 0.0 || norm >= DOMAIN_MIN_NORM);
    if (!in_domain) {
        for (uint64_t j = 0; j < dim; ++j) dst[j] = 0.0;
        *norm_out = 0.0;
    } else {
        *norm_out = norm;
    }
    return in_domain;
}

// stage_query's verdict without the copy (the same sums in the same order): a filtered batch plans its launches before it
// stages any query, and the plan has to know which jobs may take the fast path.
bool query_in_domain(const double* q, uint64_t dim)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
    uint64_t i = 0;
    for (; i + 4 <= dim; i += 4) {
        const double a = q[i], b = q[i + 1], c = q[i + 2], d = q[i + 3];
        s0 += a * a;
        s1 += b * b;
        s2 += c * c;
        s3 += d * d;
        const double fa = std::fabs(a), fb = std::fabs(b), fc = std::fabs(c), fd = std::fabs(d);
        m0 = fa > m0 ? fa : m0;
        m1 = fb > m1 ? fb : m1;
        m2 = fc > m2 ? fc : m2;
        m3 = fd > m3 ? fd : m3;
    }
    for (; i < dim; ++i) {
        const double a = q[i];
        s0 += a * a;
        const double fa = std::fabs(a);
        m0 = fa > m0 ? fa : m0;
    }
    const double qq = (s0 + s1) + (s2 + s3);
    const double m01 = m0 > m1 ? m0 : m1, m23 = m2 > m3 ? m2 : m3;
    const double qmax = m01 > m23 ? m01 : m23;
    const double norm = std::sqrt(qq);
    const bool finite = qq == qq && qmax <= 1.797693134862315708e308 && norm <= 1.797693134862315708e308;
    return finite && qmax <= DOMAIN_MAX_ABS && (norm == 0.0 || norm >= DOMAIN_MIN_NORM);
}

// The single-query entry points stage their query here instead: ws->h_q64 = the f64 values, then the norm.  Two staging
// functions because they differ in what the certified bounds see.  This one sums the squares sequentially -- the order the
// filter audits restate (tests/native/filter_audit.hip) -- and keeps the raw values of a query outside the domain, which
// the exact route reads; stage_query's four accumulators round the norm differently in the last bit, and it zeroes.
struct StagedQuery {
    double norm;
    bool in_domain;
};
StagedQuery stage_single_query(Workspace* ws, const double* query, uint64_t dim)
{
    double qq = 0.0, qmax = 0.0;
    bool finite = true;
    for (uint64_t i = 0; i < dim; ++i) {
        const double v = query[i];
        ws->h_q64[i] = v;
        qq += v * v;
        const double av = std::fabs(v);
        if (!(av <= 1.797693134862315708e308)) finite = false;
        if (av > qmax) qmax = av;
    }
    const double norm = std::sqrt(qq);
    ws->h_q64[dim] = norm;
    return {norm, finite && qmax <= DOMAIN_MAX_ABS && (norm == 0.0 || norm >= DOMAIN_MIN_NORM)};
}
}  // namespace

int GpuFlatIndex::create(uint64_t dim, int device, GpuFlatIndex** out)
{
    if (!out) return ERR_INVALID_ARG;
    *out = nullptr;
    if (dim == 0 || dim > 0x0FFFFFFFull) {
        set_last_error("dimension must be in [1, 2^28)");
        return ERR_INVALID_ARG;
    }
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) {
        set_last_error("no HIP device visible: vectorlite_amd has no CPU fallback");
        return ERR_DEVICE;
    }
    if (device < 0 || device >= n_dev) {
        set_last_error("device ordinal out of range");
        return ERR_DEVICE;
    }
    VL_HIP(hipSetDevice(device));
    std::unique_ptr<GpuFlatIndex> idx(new GpuFlatIndex(dim, device));
    VL_HIP(hipStreamCreateWithFlags(&idx->mut_stream_, hipStreamNonBlocking));
    VL_TRY(dev_alloc(&idx->d_stats_, 1));
    VL_HIP(hipMemsetAsync(idx->d_stats_, 0, sizeof(IngestStats), idx->mut_stream_));
    VL_HIP(hipStreamSynchronize(idx->mut_stream_));
    // VL_SINGLE_FILTER=f32|bf16|auto|i8: the single-query filter a handle starts with (auto when unset or unrecognised)
    idx->set_single_filter(parse_single_filter(getenv("VL_SINGLE_FILTER"), FILTER_AUTO));
    if (const char* mb = getenv("VL_SINGLE_FILTER_MIN_MB")) {
        if (*mb) idx->set_single_filter_min_bytes(std::strtoull(mb, nullptr, 10) << 20);
    }
    if (const char* mb = getenv("VL_SINGLE_FILTER_I8_MIN_MB")) {
        if (*mb) idx->set_single_filter_i8_min_bytes(std::strtoull(mb, nullptr, 10) << 20);
    }
    // Concurrent single searches share slab passes by default (the reference's many-readers model, src/client.rs:398):
    // window 0, so a lone caller leads a pass of one = the plain single-search path.  VL_COALESCE=0 starts handles with it off.
    {
        const char* ce = getenv("VL_COALESCE");
        if (!(ce && ce[0] == '0')) idx->set_coalescing(COALESCE_DEFAULT_BATCH, 0);
    }
    *out = idx.release();
    return OK;
}

// ---------------------------------------------------------------------------------------------
// workspace pools, one per (device, dimension), shared by the handles (flat_index.hpp)
// ---------------------------------------------------------------------------------------------
namespace {
struct PoolKey {
    int device;
    uint64_t dim;
    bool operator<(const PoolKey& o) const { return device != o.device ? device < o.device : dim < o.dim; }
};
std::mutex g_pools_mu;
// never destroyed: a pool that outlives main() (handles leaked by a host that exits without destroying them) must not
// call into a HIP runtime that is already gone from a static destructor
auto& g_pools = *new std::map<PoolKey, std::unique_ptr<WorkspacePool>>();
}  // namespace

WorkspacePool* GpuFlatIndex::attach_pool(int device, uint64_t dim)
{
    std::lock_guard<std::mutex> g(g_pools_mu);
    auto& slot = g_pools[PoolKey{device, dim}];
    if (!slot) slot.reset(new WorkspacePool());
    slot->users += 1;
    return slot.get();
}

void GpuFlatIndex::detach_pool(int device, uint64_t dim)
{
    std::unique_ptr<WorkspacePool> last;
    {
        std::lock_guard<std::mutex> g(g_pools_mu);
        auto it = g_pools.find(PoolKey{device, dim});
        if (it == g_pools.end()) return;
        if (--it->second->users == 0) {
            last = std::move(it->second);
            g_pools.erase(it);
        }
    }
    if (last) {
        (void)hipSetDevice(device);
        last->all.clear();  // ~Workspace frees its buffers
    }
}

GpuFlatIndex::~GpuFlatIndex()
{
    (void)hipSetDevice(device_);
    if (ws_pool_) detach_pool(device_, dim_);
    if (mut_stream_) (void)hipStreamSynchronize(mut_stream_);
    void* dev[] = {d_master_, d_slab_, d_inv_norm_, d_flags_, d_stats_, d_bounce_, d_slab16_, d_sqnorm_, d_norm16_, d_slab16f_, d_ids_,
                   d_slab8_, d_sr8_, d_norm8_};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (mut_stream_) (void)hipStreamDestroy(mut_stream_);
}

uint64_t GpuFlatIndex::len() const
{
    std::shared_lock<RwLock> lk(mu_);
    return ids_.size();
}

int GpuFlatIndex::reserve(uint64_t n_rows)
{
    std::unique_lock<RwLock> lk(mu_);
    VL_HIP(hipSetDevice(device_));
    return ensure_capacity(n_rows);
}

void GpuFlatIndex::truncate(uint64_t n_rows)
{
    std::unique_lock<RwLock> lk(mu_);
    if (n_rows >= ids_.size()) return;
    for (uint64_t p = n_rows; p < row_flags_.size(); ++p)
        if (row_flags_[p] & ROW_OUT_OF_DOMAIN) --n_out_of_domain_;
    ids_.resize(n_rows);
    row_flags_.resize(n_rows);
    ++mutations_;
    id_counts_valid_ = false;  // rebuilt on demand from ids_
    if (slab16_rows_ > n_rows) slab16_rows_ = n_rows;
    if (slab16f_rows_ > n_rows) slab16f_rows_ = n_rows;
    if (slab8_rows_ > n_rows) slab8_rows_ = n_rows;
    if (d_ids_rows_ > n_rows) d_ids_rows_ = n_rows;
}

int GpuFlatIndex::ensure_capacity(uint64_t rows)
{
    if (rows <= cap_) return OK;
    if (rows >= 0xFFFFFFF0ull) {
        set_last_error("row count exceeds the u32 position space");
        return ERR_INVALID_ARG;
    }
    // The bf16 copies of the slab are rebuilt on demand by the next large batch: they go first -- at tens of millions of
    // rows they are tens of gigabytes the growth below can use.
    if (d_norm16_) {
        if (d_slab16_) (void)hipFree(d_slab16_);
        if (d_slab16f_) (void)hipFree(d_slab16f_);
        (void)hipFree(d_sqnorm_);
        (void)hipFree(d_norm16_);
        d_slab16_ = nullptr;
        d_slab16f_ = nullptr;
        d_sqnorm_ = nullptr;
        d_norm16_ = nullptr;
        slab16_rows_ = 0;
        slab16f_rows_ = 0;
    }
    if (d_slab8_) {  // ... and so does the int8 copy of the single-query filter
        (void)hipFree(d_slab8_);
        (void)hipFree(d_sr8_);
        (void)hipFree(d_norm8_);
        d_slab8_ = nullptr;
        d_sr8_ = nullptr;
        d_norm8_ = nullptr;
        slab8_rows_ = 0;
    }
    const uint64_t n = ids_.size();
    // One array at a time: allocate the larger one, copy, free the old one.  The transient need is the index as it stands
    // plus the LARGEST new array (the f64 master), not plus all four -- an index that was never reserve()d can grow to
    // well past half of the card (growing all four at once failed at 34 M x 384 rows with 138 GiB free).  An array that
    // has grown keeps its capacity if a later one fails: cap_ (the minimum) moves only when all four hold new_cap rows.
    auto grow = [&](auto*& ptr, uint64_t& cap_arr, uint64_t new_cap, uint64_t per_row) -> int {
        if (cap_arr >= new_cap) return OK;
        using T = std::remove_reference_t<decltype(*ptr)>;
        T* fresh = nullptr;
        VL_TRY(dev_alloc(&fresh, new_cap * per_row));
        hipError_t ce = hipSuccess;
        if (n && ptr) ce = hipMemcpyAsync(fresh, ptr, n * per_row * sizeof(T), hipMemcpyDeviceToDevice, mut_stream_);
        const hipError_t se = hipStreamSynchronize(mut_stream_);
        if (ce == hipSuccess) ce = se;
        if (ce != hipSuccess) {  // the old array stays the index; the new one is not leaked
            (void)hipGetLastError();
            (void)hipFree(fresh);
            set_last_error(std::string("growing the row store failed: ") + hipGetErrorString(ce));
            return ERR_DEVICE;
        }
        if (ptr) (void)hipFree(ptr);
        ptr = fresh;
        cap_arr = new_cap;
        return OK;
    };
    auto attempt = [&](uint64_t new_cap) -> int {
        VL_TRY(grow(d_master_, cap_master_, new_cap, dim_ ? dim_ : 1));
        VL_TRY(grow(d_slab_, cap_slab_, new_cap, ld_ ? ld_ : 4));
        VL_TRY(grow(d_inv_norm_, cap_inv_, new_cap, 1));
        VL_TRY(grow(d_flags_, cap_flags_, new_cap, 1));
        cap_ = std::min(std::min(cap_master_, cap_slab_), std::min(cap_inv_, cap_flags_));
        return OK;
    };
    const uint64_t grown = cap_ < (1ull << 20) ? cap_ * 2 : cap_ + cap_ / 2;
    const uint64_t geometric = std::max<uint64_t>({rows, grown, 1024});
    int rc = attempt(geometric);
    if (rc == ERR_OOM && rows < geometric) rc = attempt(rows);  // no room for the geometric step: exactly what was asked for
    return rc;
}

// Rows [first, first+n) of d_master_ are in place: derive slab / inv_norm / flags / stats.
int GpuFlatIndex::ingest_range(uint64_t first, uint64_t n)
{
    if (n == 0) return OK;
    VL_HIP(launch_ingest(mut_stream_, d_master_ + first * dim_, d_slab_ + first * ld_, d_inv_norm_ + first,
                         d_flags_ + first, d_stats_, n, (uint32_t)dim_, ld_));
    std::vector<uint8_t> fl(n);
    IngestStats st;
    VL_HIP(hipMemcpyAsync(fl.data(), d_flags_ + first, n, hipMemcpyDeviceToHost, mut_stream_));
    VL_HIP(hipMemcpyAsync(&st, d_stats_, sizeof(st), hipMemcpyDeviceToHost, mut_stream_));
    VL_HIP(hipStreamSynchronize(mut_stream_));
    row_flags_.resize(first + n);
    for (uint64_t i = 0; i < n; ++i) {
        row_flags_[first + i] = fl[i];
        if (fl[i] & ROW_OUT_OF_DOMAIN) ++n_out_of_domain_;
    }
    double mn;
    static_assert(sizeof(mn) == sizeof(st.max_norm_bits), "f64 bits");
    std::memcpy(&mn, &st.max_norm_bits, sizeof(mn));
    if (mn > max_row_norm_) max_row_norm_ = mn;
    return OK;
}

void GpuFlatIndex::rebuild_id_counts() const
{
    id_counts_.clear();
    id_counts_.reserve(ids_.size() * 2);
    for (uint64_t id : ids_) ++id_counts_[id];
    id_counts_valid_ = true;
}

// ---------------------------------------------------------------------------------------------
// add / delete
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::add(uint64_t id, const double* values, uint64_t len)
{
    if (len != dim_) {  // src/index/flat.rs:83-85
        set_dim_mismatch(dim_, len);
        set_last_error("Vector dimension mismatch");
        return ERR_DIM_MISMATCH;
    }
    if (!values && dim_) return ERR_INVALID_ARG;
    return add_bulk(&id, values, 1, /*validate=*/true, /*values_on_device=*/false);
}

int GpuFlatIndex::add_bulk(const uint64_t* ids, const double* values, uint64_t n, bool validate,
                           bool values_on_device, int src_device)
{
    if (n == 0) return OK;
    if (!ids || (!values && dim_)) return ERR_INVALID_ARG;
    std::unique_lock<RwLock> lk(mu_);
    VL_HIP(hipSetDevice(device_));
    return add_bulk_locked(ids, values, n, validate, values_on_device, src_device);
}

int GpuFlatIndex::add_bulk_locked(const uint64_t* ids, const double* values, uint64_t n, bool validate, bool values_on_device,
                                  int src_device)
{
    uint64_t n_take = n;
    int rc_after = OK;
    if (validate) {  // n sequential add() calls: stop at the first duplicate id (src/index/flat.rs:86-88)
        if (!id_counts_valid_) rebuild_id_counts();
        for (uint64_t i = 0; i < n; ++i) {
            auto it = id_counts_.find(ids[i]);
            if (it != id_counts_.end() && it->second > 0) {
                n_take = i;
                rc_after = ERR_DUP_ID;
                set_last_error("Vector ID " + std::to_string(ids[i]) + " already exists");
                break;
            }
            ++id_counts_[ids[i]];
        }
    } else {
        id_counts_valid_ = false;  // FlatIndex::new validates nothing; counts are rebuilt on demand
    }
    if (n_take == 0) return rc_after;

    const uint64_t first = ids_.size();
    int rc = ensure_capacity(first + n_take);
    if (rc == OK && dim_) {
        hipError_t e;
        if (values_on_device && src_device >= 0 && src_device != device_)
            e = hipMemcpyPeerAsync(d_master_ + first * dim_, device_, values, src_device, n_take * dim_ * sizeof(double),
                                   mut_stream_);
        else
            e = hipMemcpyAsync(d_master_ + first * dim_, values, n_take * dim_ * sizeof(double),
                               values_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, mut_stream_);
        if (e != hipSuccess) {
            set_last_error(std::string("hipMemcpyAsync(rows): ") + hipGetErrorString(e));
            rc = ERR_DEVICE;
        }
    }
    if (rc == OK) rc = ingest_range(first, n_take);
    if (rc != OK) {
        if (validate)  // roll the id bookkeeping back
            for (uint64_t i = 0; i < n_take; ++i) --id_counts_[ids[i]];
        return rc;
    }
    ids_.insert(ids_.end(), ids, ids + n_take);
    ++mutations_;
    return rc_after;
}

// In-place update / upsert.  Nothing moves: ids_, the row order, mutations_ and the watermarks of the
// lazy copies stay as they are; what changes is the f64 master row and every copy derived from it that exists for the row.
int GpuFlatIndex::update(uint64_t id, const double* values, uint64_t len)
{
    if (len != dim_ || (!values && dim_)) {
        for (auto& v : last_update_) v.store(0, std::memory_order_relaxed);  // a refused call did nothing
        if (len == dim_) return ERR_INVALID_ARG;
        set_dim_mismatch(dim_, len);
        set_last_error("Vector dimension mismatch");
        return ERR_DIM_MISMATCH;
    }
    return update_bulk(&id, values, 1, /*insert_missing=*/false, nullptr, nullptr);
}

int GpuFlatIndex::update_bulk(const uint64_t* ids, const double* values, uint64_t n, bool insert_missing, uint64_t* out_updated,
                              uint64_t* out_inserted)
{
    if (out_updated) *out_updated = 0;
    if (out_inserted) *out_inserted = 0;
    std::unique_lock<RwLock> lk(mu_);
    for (auto& v : last_update_) v.store(0, std::memory_order_relaxed);  // a call that does nothing reads as all zero
    if (n && (!ids || (!values && dim_))) {
        set_last_error("update_bulk: null ids or values with n > 0");
        return ERR_INVALID_ARG;
    }
    if (n == 0) return OK;

    // every refusal is decided here, before the device is touched
    const UpdatePlan plan = update_plan(ids_.data(), ids_.size(), ids, n, insert_missing);
    if (plan.refused) {
        set_last_error("Vector ID " + std::to_string(plan.missing_id) + " does not exist");
        return ERR_NOT_FOUND;
    }
    VL_HIP(hipSetDevice(device_));
    const uint64_t m = plan.pos.size(), n_add = plan.append_ids.size();
    // room for the appended rows first: growth is the one step that can run out of memory, and it changes no row
    if (n_add) VL_TRY(ensure_capacity(ids_.size() + n_add));

    uint64_t in_copy[3] = {0, 0, 0}, chunks = 0, micros = 0;
    if (m && dim_) {
        const size_t want_bytes = bounce_want_ ? bounce_want_ : BOUNCE_BYTES;
        const uint64_t stage_rows = std::min<uint64_t>(update_stage_rows(want_bytes, dim_), m);
        const size_t need_bytes = std::max<size_t>(want_bytes, update_stage_bytes(stage_rows, dim_));
        if (d_bounce_ && bounce_bytes_ < need_bytes) {
            (void)hipFree(d_bounce_);
            d_bounce_ = nullptr;
            bounce_bytes_ = 0;
        }
        if (!d_bounce_) {
            VL_HIP(hipMalloc(&d_bounce_, need_bytes));
            bounce_bytes_ = need_bytes;
        }
        char* stage = static_cast<char*>(d_bounce_);
        double* d_rows = reinterpret_cast<double*>(stage);
        uint32_t* d_pos = reinterpret_cast<uint32_t*>(stage + update_stage_pos_offset(stage_rows, dim_));
        uint8_t* d_newfl = reinterpret_cast<uint8_t*>(stage + update_stage_flag_offset(stage_rows, dim_));
        std::vector<double> h_rows(stage_rows * dim_);
        std::vector<uint32_t> h_pos(stage_rows);
        std::vector<uint8_t> h_fl(stage_rows);
        // the lazy copies as they stand (mu_ is held exclusively: no search is converting rows)
        struct Copy {
            int kind;
            void* base;
            float *a, *b;
            uint64_t rows_done;
        } const copies[3] = {{UPDATE_COPY_BF16, d_slab16_, d_norm16_, d_sqnorm_, d_slab16_ ? slab16_rows_ : 0},
                             {UPDATE_COPY_BF16_FRAG, d_slab16f_, d_norm16_, d_sqnorm_, d_slab16f_ ? slab16f_rows_ : 0},
                             {UPDATE_COPY_I8, d_slab8_, d_sr8_, d_norm8_, d_slab8_ ? slab8_rows_ : 0}};
        const auto t0 = std::chrono::steady_clock::now();
        for (const auto& cut : update_chunks(m, stage_rows)) {
            const uint64_t c = cut.second - cut.first;
            for (uint64_t j = 0; j < c; ++j) {
                std::memcpy(&h_rows[j * dim_], values + plan.src[cut.first + j] * dim_, dim_ * sizeof(double));
                h_pos[j] = (uint32_t)plan.pos[cut.first + j];
            }
            VL_HIP(hipMemcpyAsync(d_rows, h_rows.data(), c * dim_ * sizeof(double), hipMemcpyHostToDevice, mut_stream_));
            VL_HIP(hipMemcpyAsync(d_pos, h_pos.data(), c * sizeof(uint32_t), hipMemcpyHostToDevice, mut_stream_));
            VL_HIP(launch_update_rows(mut_stream_, d_rows, d_pos, (uint32_t)c, d_master_, d_slab_, d_inv_norm_, d_flags_, d_newfl,
                                      d_stats_, (uint32_t)dim_, ld_));
            for (const Copy& cp : copies)
                if (cp.base && cp.rows_done)
                    VL_HIP(launch_update_copies(mut_stream_, cp.kind, d_rows, d_pos, (uint32_t)c, cp.rows_done, (uint32_t)dim_, cp.base,
                                                cp.a, cp.b));
            VL_HIP(hipMemcpyAsync(h_fl.data(), d_newfl, c, hipMemcpyDeviceToHost, mut_stream_));
            VL_HIP(hipStreamSynchronize(mut_stream_));  // the host buffers are reused by the next chunk
            for (uint64_t j = 0; j < c; ++j) {
                const uint64_t p = h_pos[j];
                const bool was = row_flags_[p] & ROW_OUT_OF_DOMAIN, is = h_fl[j] & ROW_OUT_OF_DOMAIN;
                if (was && !is) --n_out_of_domain_;
                if (!was && is) ++n_out_of_domain_;
                row_flags_[p] = h_fl[j];
                for (int k = 0; k < 3; ++k)
                    if (copies[k].base && p < copies[k].rows_done) ++in_copy[k];
            }
            ++chunks;
        }
        IngestStats st;
        VL_HIP(hipMemcpyAsync(&st, d_stats_, sizeof(st), hipMemcpyDeviceToHost, mut_stream_));
        VL_HIP(hipStreamSynchronize(mut_stream_));
        micros = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        double mn;
        std::memcpy(&mn, &st.max_norm_bits, sizeof(mn));
        if (mn > max_row_norm_) max_row_norm_ = mn;  // an upper bound over rows ever stored: only ever raised
    }
    if (n_add) {  // the absent ids, once each, through the add path (ids_ grows, mutations_ is bumped once)
        std::vector<double> rows(n_add * dim_);
        for (uint64_t j = 0; j < n_add; ++j)
            if (dim_) std::memcpy(&rows[j * dim_], values + plan.append_src[j] * dim_, dim_ * sizeof(double));
        VL_TRY(add_bulk_locked(plan.append_ids.data(), rows.data(), n_add, /*validate=*/true, /*values_on_device=*/false, -1));
    }
    const uint64_t st7[7] = {m, n_add, in_copy[0], in_copy[1], in_copy[2], chunks, micros};
    for (int i = 0; i < 7; ++i) last_update_[i].store(st7[i], std::memory_order_relaxed);
    if (out_updated) *out_updated = m;
    if (out_inserted) *out_inserted = n_add;
    return OK;
}

// Order-preserving removal of one row (Vec::retain, src/index/flat.rs:94): rows behind it move up
// by one.  Overlapping device ranges are moved through a bounce buffer in ascending chunks.
int GpuFlatIndex::remove_position(uint64_t pos)
{
    const uint64_t n = ids_.size();
    const uint64_t tail = n - pos - 1;
    if (tail) {
        if (!d_bounce_) {
            VL_HIP(hipMalloc(&d_bounce_, BOUNCE_BYTES));
            bounce_bytes_ = BOUNCE_BYTES;
        }
        struct Buf {
            char* base;
            size_t row_bytes;
        } bufs[] = {{reinterpret_cast<char*>(d_master_), dim_ * sizeof(double)},
                    {reinterpret_cast<char*>(d_slab_), ld_ * sizeof(float)},
                    {reinterpret_cast<char*>(d_inv_norm_), sizeof(float)},
                    {reinterpret_cast<char*>(d_flags_), 1}};
        for (const Buf& b : bufs) {
            if (b.row_bytes == 0) continue;
            char* dst = b.base + pos * b.row_bytes;
            const char* src = dst + b.row_bytes;
            const size_t total = tail * b.row_bytes;
            for (size_t off = 0; off < total; off += bounce_bytes_) {
                const size_t c = std::min(bounce_bytes_, total - off);
                VL_HIP(hipMemcpyAsync(d_bounce_, src + off, c, hipMemcpyDeviceToDevice, mut_stream_));
                VL_HIP(hipMemcpyAsync(dst + off, d_bounce_, c, hipMemcpyDeviceToDevice, mut_stream_));
            }
        }
        VL_HIP(hipStreamSynchronize(mut_stream_));
    }
    if (row_flags_[pos] & ROW_OUT_OF_DOMAIN) --n_out_of_domain_;
    if (slab16_rows_ > pos) slab16_rows_ = pos;  // rows behind the hole are re-converted on demand
    if (slab16f_rows_ > pos) slab16f_rows_ = pos;
    if (slab8_rows_ > pos) slab8_rows_ = pos;
    if (d_ids_rows_ > pos) d_ids_rows_ = pos;    // ... and the device id table re-uploaded from there
    ids_.erase(ids_.begin() + pos);
    row_flags_.erase(row_flags_.begin() + pos);
    ++mutations_;
    return OK;
}

int GpuFlatIndex::remove(uint64_t id) { return remove_report(id, nullptr); }

bool GpuFlatIndex::contains(uint64_t id) const
{
    std::unique_lock<RwLock> lk(mu_);  // may rebuild the table
    if (!id_counts_valid_) rebuild_id_counts();
    auto it = id_counts_.find(id);
    return it != id_counts_.end() && it->second > 0;
}

int GpuFlatIndex::find_first(uint64_t id, uint64_t* out_pos) const
{
    std::shared_lock<RwLock> lk(mu_);
    auto it = std::find(ids_.begin(), ids_.end(), id);
    if (it == ids_.end()) return ERR_NOT_FOUND;
    if (out_pos) *out_pos = (uint64_t)(it - ids_.begin());
    return OK;
}

int GpuFlatIndex::get_row_at(uint64_t pos, double* out) const
{
    if (!out && dim_) return ERR_INVALID_ARG;
    std::shared_lock<RwLock> lk(mu_);
    if (pos >= ids_.size()) return ERR_NOT_FOUND;
    if (dim_) {
        VL_HIP(hipSetDevice(device_));
        VL_HIP(hipMemcpy(out, d_master_ + pos * dim_, dim_ * sizeof(double), hipMemcpyDeviceToHost));
    }
    return OK;
}

int GpuFlatIndex::remove_report(uint64_t id, std::vector<uint64_t>* removed_positions)
{
    std::unique_lock<RwLock> lk(mu_);
    VL_HIP(hipSetDevice(device_));
    // retain(|e| e.id != id): every matching row goes, highest position first
    for (uint64_t p = ids_.size(); p-- > 0;) {
        if (ids_[p] == id) {
            VL_TRY(remove_position(p));
            if (removed_positions) removed_positions->push_back(p);
            if (id_counts_valid_) {
                auto it = id_counts_.find(id);
                if (it != id_counts_.end() && it->second > 0) --it->second;
            }
        }
    }
    return OK;  // absent id is Ok(()) (src/index/flat.rs:93-96)
}

int GpuFlatIndex::set_delete_bounce(uint64_t bytes)
{
    std::unique_lock<RwLock> lk(mu_);
    const size_t widest = std::max<size_t>({dim_ * sizeof(double), ld_ * sizeof(float), 1});
    bounce_want_ = bytes ? std::max<size_t>((size_t)bytes, widest) : 0;
    const size_t want = bounce_want_ ? bounce_want_ : BOUNCE_BYTES;
    if (d_bounce_ && bounce_bytes_ < want) {  // allocated again, large enough, by the next delete
        VL_HIP(hipSetDevice(device_));
        (void)hipFree(d_bounce_);
        d_bounce_ = nullptr;
        bounce_bytes_ = 0;
    }
    return OK;
}

// n deletes at once: Vec::retain (src/index/flat.rs:93-96) applied n times is one order-preserving compaction.  One walk over
// ids_ finds the rows, delete_plan.hpp cuts each device array's moved part into segments, k_move_rows moves them; the host
// bookkeeping follows once the device work is known to have completed.
int GpuFlatIndex::remove_bulk(const uint64_t* ids, uint64_t n, std::vector<uint64_t>* removed_positions, uint64_t* out_rows)
{
    if (out_rows) *out_rows = 0;
    if (removed_positions) removed_positions->clear();
    if (n && !ids) return ERR_INVALID_ARG;
    std::unique_lock<RwLock> lk(mu_);
    for (auto& v : last_delete_) v.store(0, std::memory_order_relaxed);  // a call that removes nothing reads as all zero
    if (n == 0) return OK;
    VL_HIP(hipSetDevice(device_));

    const uint64_t rows_before = ids_.size();
    if (rows_before >= 0xFFFFFFF0ull) {  // the plan's keys and the kernel's row numbers are u32 (ensure_capacity's limit)
        set_last_error("row count exceeds the u32 position space");
        return ERR_INVALID_ARG;
    }
    std::vector<uint64_t> gone;  // ascending
    {
        // The listed ids as an open-addressing table (a power of two of slots, at most half full, linear probing; the id
        // ~0 is the empty slot's mark and is remembered beside it), behind a bitmap of the same hash's top bits -- 8 bits
        // per listed id at least -- that answers for most of the rows that stay without a probe of the table.
        constexpr uint64_t EMPTY = ~0ull;
        int log2_slots = 4, log2_bits = 10;
        while ((1ull << log2_slots) < 2 * n) ++log2_slots;
        while (log2_bits < 30 && (1ull << log2_bits) < 8 * n) ++log2_bits;
        std::vector<uint64_t> table((size_t)1 << log2_slots, EMPTY), maybe((size_t)1 << (log2_bits - 6), 0);
        const uint64_t mask = table.size() - 1;
        bool want_empty_mark = false;
        const auto hash = [](uint64_t id) { return id * 0x9E3779B97F4A7C15ull; };
        for (uint64_t i = 0; i < n; ++i) {
            if (ids[i] == EMPTY) {
                want_empty_mark = true;
                continue;
            }
            const uint64_t h = hash(ids[i]), b = h >> (64 - log2_bits);
            maybe[b >> 6] |= 1ull << (b & 63);
            uint64_t s = h >> (64 - log2_slots);
            while (table[s] != EMPTY && table[s] != ids[i]) s = (s + 1) & mask;
            table[s] = ids[i];
        }
        for (uint64_t p = 0; p < rows_before; ++p) {
            const uint64_t id = ids_[p];
            if (id == EMPTY) {
                if (want_empty_mark) gone.push_back(p);
                continue;
            }
            const uint64_t h = hash(id), b = h >> (64 - log2_bits);
            if (!((maybe[b >> 6] >> (b & 63)) & 1)) continue;
            uint64_t s = h >> (64 - log2_slots);
            while (table[s] != EMPTY && table[s] != id) s = (s + 1) & mask;
            if (table[s] == id) gone.push_back(p);
        }
    }
    const uint64_t m = gone.size();
    if (m == 0) return OK;  // absent ids are Ok(()), and nothing changed
    const uint64_t rows_after = rows_before - m, first = gone[0];

    uint64_t launches = 0, bounced = 0, bytes_written = 0, micros = 0;
    if (first < rows_after) {  // rows behind a hole survive: they move up
        const size_t want_bytes = bounce_want_ ? bounce_want_ : BOUNCE_BYTES;
        if (d_bounce_ && bounce_bytes_ < want_bytes) {
            (void)hipFree(d_bounce_);
            d_bounce_ = nullptr;
            bounce_bytes_ = 0;
        }
        if (!d_bounce_) {
            VL_HIP(hipMalloc(&d_bounce_, want_bytes));
            bounce_bytes_ = want_bytes;
        }
        const std::vector<uint32_t> keys = delete_keys(gone);
        struct DevKeys {  // the removed list on the device for the length of this call
            uint32_t* p = nullptr;
            ~DevKeys()
            {
                if (p) (void)hipFree(p);
            }
        } d_keys;
        VL_TRY(dev_alloc(&d_keys.p, keys.size()));
        VL_HIP(hipMemcpyAsync(d_keys.p, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, mut_stream_));
        struct Buf {
            char* base;
            size_t row_bytes;
        } bufs[] = {{reinterpret_cast<char*>(d_master_), dim_ * sizeof(double)},
                    {reinterpret_cast<char*>(d_slab_), ld_ * sizeof(float)},
                    {reinterpret_cast<char*>(d_inv_norm_), sizeof(float)},
                    {reinterpret_cast<char*>(d_flags_), 1}};
        const auto t0 = std::chrono::steady_clock::now();
        for (const Buf& b : bufs) {
            if (b.row_bytes == 0) continue;
            for (const DeleteSegment& sg : delete_plan(rows_before, keys, want_bytes / b.row_bytes)) {
                const uint64_t cnt = sg.dst_end - sg.dst_begin;
                char* place = b.base + sg.dst_begin * b.row_bytes;
                VL_HIP(launch_move_rows(mut_stream_, b.base, sg.direct ? place : static_cast<char*>(d_bounce_), b.row_bytes, d_keys.p,
                                        (uint32_t)sg.shift_begin, (uint32_t)sg.shift_end, sg.dst_begin, cnt));
                if (sg.direct) {
                    ++launches;
                } else {
                    VL_HIP(hipMemcpyAsync(place, d_bounce_, cnt * b.row_bytes, hipMemcpyDeviceToDevice, mut_stream_));
                    ++bounced;
                }
                bytes_written += cnt * b.row_bytes * (sg.direct ? 1 : 2);
            }
        }
        VL_HIP(hipStreamSynchronize(mut_stream_));
        micros = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    }

    // the device arrays are compacted: now the host's
    {
        // the runs of kept rows between the holes move up as blocks
        uint64_t w = first;
        for (size_t gi = 0; gi < gone.size(); ++gi) {
            const uint64_t p = gone[gi];
            if (row_flags_[p] & ROW_OUT_OF_DOMAIN) --n_out_of_domain_;
            if (id_counts_valid_) {
                auto it = id_counts_.find(ids_[p]);
                if (it != id_counts_.end() && it->second > 0) --it->second;
            }
            const uint64_t run_end = gi + 1 < gone.size() ? gone[gi + 1] : rows_before, run = run_end - (p + 1);
            if (run) {
                std::memmove(&ids_[w], &ids_[p + 1], run * sizeof(uint64_t));
                std::memmove(&row_flags_[w], &row_flags_[p + 1], run);
                w += run;
            }
        }
        ids_.resize(rows_after);
        row_flags_.resize(rows_after);
    }
    if (slab16_rows_ > first) slab16_rows_ = first;  // rows behind the first hole are re-converted on demand
    if (slab16f_rows_ > first) slab16f_rows_ = first;
    if (slab8_rows_ > first) slab8_rows_ = first;
    if (d_ids_rows_ > first) d_ids_rows_ = first;
    ++mutations_;
    const uint64_t st[6] = {m, rows_after - first, launches, bounced, bytes_written, micros};
    for (int i = 0; i < 6; ++i) last_delete_[i].store(st[i], std::memory_order_relaxed);
    if (out_rows) *out_rows = m;
    if (removed_positions) *removed_positions = std::move(gone);
    return OK;
}

// ---------------------------------------------------------------------------------------------
// workspaces
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::prepare_ws(Workspace* ws) const
{
    ws->device = device_;
    VL_HIP(hipStreamCreateWithFlags(&ws->stream, hipStreamNonBlocking));
    // staged queries: up to SCAN_BATCH_QB rows of dim f64, followed by their norms
    const size_t qn = (size_t)SCAN_BATCH_QB * (dim_ + 1) + 8;
    ws->q_cap = qn;
    VL_TRY(dev_alloc(&ws->d_q64, qn));
    VL_TRY(pinned_alloc(&ws->h_q64, qn));
    VL_TRY(dev_alloc(&ws->d_partials, PARTIALS32_ENTRIES));
    VL_TRY(dev_alloc(&ws->d_partials64, PARTIALS64_ENTRIES));
    VL_TRY(dev_alloc(&ws->d_result, SELECT_MAX_ROUNDS));
    VL_TRY(pinned_alloc(&ws->h_result, SELECT_MAX_ROUNDS > SCAN_BATCH_QB ? SELECT_MAX_ROUNDS : SCAN_BATCH_QB));
    VL_TRY(dev_alloc(&ws->d_nan, 1));
    VL_TRY(pinned_alloc(&ws->h_nan, 1));
    VL_HIP(hipEventCreate(&ws->ev0));
    VL_HIP(hipEventCreate(&ws->ev1));
    return OK;
}

Workspace* GpuFlatIndex::acquire_ws() const
{
    WorkspacePool* pool = ws_pool_;
    {
        std::lock_guard<std::mutex> g(pool->mu);
        if (!pool->free_.empty()) {
            Workspace* w = pool->free_.back();
            pool->free_.pop_back();
            return w;
        }
    }
    std::unique_ptr<Workspace> w(new Workspace());
    if (prepare_ws(w.get()) != OK) return nullptr;
    Workspace* raw = w.get();
    std::lock_guard<std::mutex> g(pool->mu);
    pool->all.push_back(std::move(w));
    return raw;
}

void GpuFlatIndex::release_ws(Workspace* ws) const
{
    std::lock_guard<std::mutex> g(ws_pool_->mu);
    ws_pool_->free_.push_back(ws);
}

// A workspace borrowed for one call.  The caller records the call's status with done(); a call that failed may still have
// work of its own on the stream, which is drained before the workspace goes back.  The single-query entry points must not
// synchronise on success (their latency is a stamp poll, wait_result); the batch routes always do (sync_always), so
// they have no status to record and return without done().
class GpuFlatIndex::WsLease {
public:
    explicit WsLease(const GpuFlatIndex* self, bool sync_always = false) : self_(self), device_(self->device_), sync_always_(sync_always)
    {
        status_ = open();
    }
    ~WsLease()
    {
        if (!ws) return;
        if (sync_always_ || status_ != OK) (void)hipStreamSynchronize(ws->stream);
        self_->release_ws(ws);
    }
    WsLease(const WsLease&) = delete;
    WsLease& operator=(const WsLease&) = delete;
    int status() const { return status_; }  // of the lease itself (hipSetDevice, the pool) until done() records the call's
    int done(int rc) { return status_ = rc; }

    Workspace* ws = nullptr;

private:
    int open()
    {
        VL_HIP(hipSetDevice(device_));
        ws = self_->acquire_ws();
        return ws ? OK : ERR_DEVICE;
    }
    const GpuFlatIndex* self_;
    const int device_;
    const bool sync_always_;
    int status_ = OK;
};

namespace {
int check_metric(int metric)
{
    if (metric >= 0 && metric <= 3) return OK;
    set_last_error("unknown metric");
    return ERR_INVALID_ARG;
}
struct InFlight {  // one of the handle's single searches in flight (wait_result's spin-or-sleep choice counts them)
    std::atomic<int>& n;
    explicit InFlight(std::atomic<int>& counter) : n(counter) { n.fetch_add(1, std::memory_order_relaxed); }
    ~InFlight() { n.fetch_sub(1, std::memory_order_relaxed); }
};
}  // namespace

int GpuFlatIndex::dim_mismatch(uint64_t q_len) const
{
    set_dim_mismatch(dim_, q_len);
    set_last_error("Dimension mismatch: expected " + std::to_string(dim_) + ", got " + std::to_string(q_len));
    return ERR_DIM_MISMATCH;
}

// The checks every read-side entry point makes once its tokens are looked up, in the order callers can observe: the
// metric, then the index lock (shared: readers share it, add / delete wait, so resolved lists and positions cannot move
// under the search), then the query length (src/index/flat.rs:99-104: skipped while the index is empty).
int GpuFlatIndex::lock_for_query(int metric, uint64_t q_len, std::shared_lock<RwLock>* lk) const
{
    VL_TRY(check_metric(metric));
    *lk = std::shared_lock<RwLock>(mu_);
    if (!ids_.empty() && q_len != dim_) return dim_mismatch(q_len);
    return OK;
}

int GpuFlatIndex::resolve_if_stale(Workspace* ws, IdFilter* f, bool need_list) const
{
    std::lock_guard<std::mutex> g(f->mu);
    if (filter_stale(f)) VL_TRY(resolve_filter(ws, f));
    return need_list ? ensure_plist(ws, f) : OK;
}

int GpuFlatIndex::resolve_if_stale(Workspace* ws, GroupTable* t) const
{
    std::lock_guard<std::mutex> g(t->rows.mu);
    return t->rows.resolved_at != mutations_ ? resolve_groups(ws, t) : OK;
}

// From here on the resolutions are read only: a reader that finds them current leaves them alone, writers are shut out.
template <typename Body>
int GpuFlatIndex::run_search(GroupTable* t, IdFilter* f, Body&& body, bool need_list) const
{
    WsLease lease(this);
    if (lease.status() != OK) return lease.status();
    if (t) VL_TRY(lease.done(resolve_if_stale(lease.ws, t)));
    if (f) VL_TRY(lease.done(resolve_if_stale(lease.ws, f, need_list)));
    InFlight searching(active_searches_);
    return lease.done(body(lease.ws));
}

// One profiled scan: the time between the workspace's event pair, the bytes it streamed.  A stamp poll can return
// before the runtime has retired ev1, hence the retry; where the stream was synchronised it never triggers.
int GpuFlatIndex::account_profile(Workspace* ws, uint64_t bytes, uint64_t passes) const
{
    float ms = 0.f;
    hipError_t pe = hipEventElapsedTime(&ms, ws->ev0, ws->ev1);
    if (pe == hipErrorNotReady) {
        VL_HIP(hipEventSynchronize(ws->ev1));
        pe = hipEventElapsedTime(&ms, ws->ev0, ws->ev1);
    }
    VL_HIP(pe);
    std::lock_guard<std::mutex> g(prof_mu_);
    prof_n_ += passes;
    prof_ms_ += ms;
    prof_bytes_ += bytes;
    return OK;
}

void GpuFlatIndex::profile_enable(bool on) { profile_.store(on); }

void GpuFlatIndex::profile_read(uint64_t* n, double* ms, uint64_t* bytes)
{
    std::lock_guard<std::mutex> g(prof_mu_);
    if (n) *n = prof_n_;
    if (ms) *ms = prof_ms_;
    if (bytes) *bytes = prof_bytes_;
    prof_n_ = 0;
    prof_ms_ = 0.0;
    prof_bytes_ = 0;
}

// ---------------------------------------------------------------------------------------------
// search (src/index/flat.rs:98-119)
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::search(const double* query, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
                         uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    if (co_.enabled())
        return search_coalesced(query, q_len, k, metric, out_pos, out_ids, out_scores, out_n);
    return search_direct(query, q_len, k, metric, out_pos, out_ids, out_scores, out_n);
}

// ---------------------------------------------------------------------------------------------
// Coalescing of concurrent single-query calls (SURVEY 8(b) threading row / 8(f) f1).
// The reference serves many searches at once under RwLock::read (src/client.rs:398, one tokio
// worker each); every one of them walks the whole slab.  Here concurrent callers share slab passes:
// a caller that finds no batch in flight becomes the leader, takes every queued request with its own
// (metric, k) -- all that piled up while the previous batch was on the GPU -- and answers them with
// ONE search_batch() pass; the others sleep until their request is marked done.  Every caller still
// receives exactly what search_direct() would have returned (search_batch's contract); a batch that
// fails as a whole (e.g. a NaN score for one member) is redone one by one so errors stay per caller.
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::search_coalesced(const double* query, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
                                   uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    if (!out_n) return ERR_INVALID_ARG;
    *out_n = 0;
    {   // everything that can fail or finish without touching the slab is settled on the calling thread
        std::shared_lock<RwLock> lk(mu_);
        const uint64_t n = ids_.size();
        if (metric < 0 || metric > 3 || (n != 0 && q_len != dim_) || n == 0 || k == 0 || (!query && dim_) || !out_scores ||
            force_path_.load() != 0)
            goto direct;
    }
    {
        CoalesceReq r{query, k, metric, out_pos, out_ids, out_scores, out_n};
        co_.run(
            r, [](const CoalesceReq& a, const CoalesceReq& o) { return a.metric == o.metric && a.k == o.k; },
            [this](std::vector<CoalesceReq*>& batch) { run_coalesced(batch); });
        set_last_path(r.path);
        if (r.rc != OK) set_last_error(r.err);
        return r.rc;
    }
direct:
    return search_direct(query, q_len, k, metric, out_pos, out_ids, out_scores, out_n);
}

void GpuFlatIndex::run_coalesced(std::vector<CoalesceReq*>& batch) const
{
    auto one = [&](CoalesceReq* o) {
        o->rc = search_direct(o->query, dim_, o->k, o->metric, o->out_pos, o->out_ids, o->out_scores, o->out_n);
        o->path = last_path();
        if (o->rc != OK) o->err = last_error();
    };
    if (batch.size() == 1) {
        one(batch[0]);
        return;
    }
    // scratch and row stride use min(k, len), never the caller's raw k: k = u64::MAX would throw length_error,
    // k = 2^63 with two queries would wrap nq * k to 0 (mutators are exclusive, so len cannot move under a search)
    uint64_t n_rows;
    {
        std::shared_lock<RwLock> lk(mu_);
        n_rows = ids_.size();
    }
    const uint64_t nq = batch.size(), k = std::min<uint64_t>(batch[0]->k, n_rows);
    int rc = OK;
    try {
        std::vector<double> q(nq * dim_);
        for (uint64_t i = 0; i < nq; ++i) std::memcpy(q.data() + i * dim_, batch[i]->query, dim_ * sizeof(double));
        std::vector<uint64_t> pos(nq * k), ids(nq * k), cnt(nq);
        std::vector<double> scores(nq * k);
        rc = search_batch(q.data(), nq, dim_, k, batch[0]->metric, pos.data(), ids.data(), scores.data(), cnt.data());
        if (rc == OK) {
            const int path = last_path();
            for (uint64_t i = 0; i < nq; ++i) {
                CoalesceReq* o = batch[i];
                const uint64_t m = cnt[i];
                for (uint64_t j = 0; j < m; ++j) {
                    if (o->out_pos) o->out_pos[j] = pos[i * k + j];
                    if (o->out_ids) o->out_ids[j] = ids[i * k + j];
                    o->out_scores[j] = scores[i * k + j];
                }
                *o->out_n = m;
                o->rc = OK;
                o->path = path;
            }
            return;
        }
    } catch (...) {  // bad_alloc, length_error: answer the callers one by one instead
        rc = ERR_OOM;
    }
    for (CoalesceReq* o : batch) one(o);  // per-caller errors (src/index/flat.rs:116 panics only the offending search)
}

int GpuFlatIndex::search_direct(const double* query, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
                                uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    if (!out_n) return ERR_INVALID_ARG;
    *out_n = 0;
    std::shared_lock<RwLock> lk;
    VL_TRY(lock_for_query(metric, q_len, &lk));
    const uint64_t n = ids_.size();
    if (n == 0 || k == 0) return OK;  // truncate(0) / nothing stored
    if ((!query && dim_) || !out_scores) return ERR_INVALID_ARG;
    return run_search(nullptr, nullptr, [&](Workspace* ws) {
        return search_locked(ws, query, std::min<uint64_t>(k, n), metric, out_pos, out_ids, out_scores, out_n, false);
    });
}

// nq independent searches sharing slab passes: up to MFMA_MAX_BATCH queries per pass over the bf16 slab
// (k_mfma_scan: cosine / dot / Euclidean, dim <= 768, >= MFMA_MIN_ROWS rows), otherwise groups of SCAN_BATCH_QB
// queries per pass over the f32 slab (k_scan_batch).  Every query still gets its own exact rescoring, bound check
// and, if that fails, its own single-query or exact-path run: each row of the output is exactly what search() returns.
int GpuFlatIndex::search_batch(const double* queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric,
                               uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    if (nq == 0) return OK;
    if (!out_n) return ERR_INVALID_ARG;
    for (uint64_t i = 0; i < nq; ++i) out_n[i] = 0;
    VL_TRY(check_metric(metric));
    std::shared_lock<RwLock> lk(mu_);
    return search_batch_locked(queries, nq, q_len, k, metric, out_pos, out_ids, out_scores, out_n);
}

// the caller holds mu_ (shared) and has zeroed out_n
int GpuFlatIndex::search_batch_locked(const double* queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric,
                                      uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    const uint64_t n = ids_.size();
    if (n != 0 && q_len != dim_) return dim_mismatch(q_len);
    if (n == 0 || k == 0) return OK;
    if (!queries || !out_scores) return ERR_INVALID_ARG;
    const uint64_t k_eff = std::min<uint64_t>(k, n);

    WsLease lease(this, /*sync_always=*/true);
    if (lease.status() != OK) return lease.status();
    Workspace* const ws = lease.ws;
    hipStream_t st = ws->stream;

    // row lengths without an 8-query f32 shape can still take the MFMA filter (its bf16 slab is padded to 128)
    const bool f32_batch = scan_batch_supported(ld_);
    const bool batchable = nq > 1 && force_path_.load() == 0 && k_eff <= (uint64_t)KFAST_MAX && n_out_of_domain_ == 0;
    auto out_at = [&](uint64_t* base, uint64_t qi) { return base ? base + qi * k : nullptr; };
    auto single = [&](uint64_t qi, bool skip_fast, bool skip_bf16 = false) -> int {
        return search_locked(ws, queries + qi * dim_, k_eff, metric, out_at(out_pos, qi), out_at(out_ids, qi),
                             out_scores + qi * k, out_n + qi, skip_fast, skip_bf16);
    };
    if (!batchable) {
        for (uint64_t qi = 0; qi < nq; ++qi) VL_TRY(single(qi, false));
        return OK;
    }

    // two or more queries: bf16 MFMA candidate filter; whatever it cannot certify is redone below
    std::vector<uint8_t> done(nq, 0);
    const char* mf_env = getenv("VL_MFMA");
    const bool mfma_on = !(mf_env && mf_env[0] == '0');
    const char* mf_min = getenv("VL_MFMA_MIN_BATCH");
    const uint64_t mfma_min = mf_min && *mf_min ? (uint64_t)atoi(mf_min) : (uint64_t)MFMA_MIN_BATCH;
    if (mfma_on && nq >= mfma_min && n >= MFMA_MIN_ROWS && mfma_scan_supported((uint32_t)dim_, metric)) {
        VL_TRY(search_batch_mfma(ws, queries, nullptr, nq, k, k_eff, metric, out_pos, out_ids, out_scores, out_n, &done));
        uint64_t left = 0;
        for (uint64_t qi = 0; qi < nq; ++qi) left += done[qi] ? 0 : 1;
        if (left == 0) {
            set_last_path(PATH_FAST);
            return OK;
        }
        if (left <= 2 || !f32_batch) {  // one or two stragglers (or no 8-query f32 shape): one by one on the f32 path
            // (a bf16 filter already failed them: the single-query bf16 stage would only add a pass)
            for (uint64_t qi = 0; qi < nq; ++qi)
                if (!done[qi]) VL_TRY(single(qi, false, true));
            return OK;
        }
    }
    if (!f32_batch) {
        for (uint64_t qi = 0; qi < nq; ++qi) VL_TRY(single(qi, false));
        return OK;
    }

    // what is left (everything, or what the MFMA filter could not certify): 8 queries per f32 slab pass
    std::vector<uint64_t> todo;
    todo.reserve(nq);
    for (uint64_t qi = 0; qi < nq; ++qi)
        if (!done[qi]) todo.push_back(qi);
    const uint64_t nt = todo.size();
    const bool prof = profile_.load();
    // Up to K3_PIPE_QUERIES queries are staged at once (one H2D copy) and answered by ONE scan launch -- their groups of 8 as
    // blockIdx.y, each group one pass over the slab -- and ONE finalize launch, then one stream sync: staged, launched and
    // synchronised pass by pass a 50 000-row index answered 70-100 k Manhattan queries per second where cosine batches
    // reach millions (round 3's verdict, item 8).
    const size_t k3_words = k3_stage_words(dim_);
    VL_TRY(ensure_set(HipMem{}, {dev_buf(ws->k3_d_q64, k3_words), pinned_buf(ws->k3_h_q64, k3_words),
                                 pinned_buf(ws->k3_h_result, K3_PIPE_QUERIES)}));
    std::vector<uint8_t> in_domain((size_t)K3_PIPE_QUERIES);
    for (uint64_t base = 0; base < nt; base += K3_PIPE_QUERIES) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(K3_PIPE_QUERIES, nt - base);
        double* norms = ws->k3_h_q64 + (size_t)cnt * dim_;
        for (uint32_t j = 0; j < cnt; ++j)
            in_domain[j] = stage_query(queries + todo[base + j] * dim_, ws->k3_h_q64 + (size_t)j * dim_, dim_, &norms[j]) ? 1 : 0;
        VL_HIP(hipMemcpyAsync(ws->k3_d_q64, ws->k3_h_q64, ((size_t)cnt * dim_ + cnt) * sizeof(double), hipMemcpyHostToDevice, st));
        const double* d_norms = ws->k3_d_q64 + (size_t)cnt * dim_;
        const uint32_t passes = (cnt + SCAN_BATCH_QB - 1) / SCAN_BATCH_QB;
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        {   // ONE scan launch (groups of 8 queries as blockIdx.y: each group is one pass over the slab) and ONE finalize launch
            ScanPlan plan;
            VL_HIP(launch_scan_batch(st, metric, d_slab_, d_inv_norm_, ws->k3_d_q64, cnt, n, (uint32_t)dim_, ld_, ws->d_partials, &plan));
            if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
            VL_HIP(launch_merge_finalize(st, metric, ws->d_partials, plan.grid, (int)cnt, d_master_, ws->k3_d_q64, d_norms,
                                         (uint32_t)dim_, n, (uint32_t)k_eff, max_row_norm_, ws->k3_h_result));
        }
        VL_HIP(hipStreamSynchronize(st));
        // (the events bracket the one scan launch: `passes` slab passes side by side)
        if (prof) VL_TRY(account_profile(ws, (uint64_t)passes * n * (uint64_t)ld_ * sizeof(float), passes));
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t qi = todo[base + j];
            const SearchResultBlock& r = ws->k3_h_result[j];  // (a fallback below uses the workspace's other buffers, not these)
            const bool ok = in_domain[j] && !(r.flags & RESULT_NEEDS_EXACT) && r.n_out == k_eff;
            if (ok) {
                VL_TRY(deliver("batch fast path", ids_, &r, k_eff, out_at(out_pos, qi), out_at(out_ids, qi), out_scores + qi * k));
                out_n[qi] = k_eff;
            } else {
                VL_TRY(single(qi, true));
            }
        }
        set_last_path(PATH_FAST);
    }
    return OK;
}

// Single-query filter choice (set_single_filter, single_filter.hpp's ladder_stage).  Modes 1 and 3 keep their one-way
// switch-off; auto applies each stage's recent-outcome window, so a bad streak pauses it and the periodic probes bring
// it back.
bool GpuFlatIndex::bf16_first(uint64_t n, bool masked) const
{
    const int mode = single_filter_.load(std::memory_order_relaxed);
    const bool ok = !(mode == FILTER_AUTO && auto_unavailable_.load(std::memory_order_relaxed));
    return ladder_stage(
        FILTER_BF16, mode, ok, n * (uint64_t)ld_ * sizeof(float), auto_min_bytes_,
        [&] {
            return forced_stage_on((masked ? mask_bf16_tries_ : bf16_tries_).load(std::memory_order_relaxed),
                                   (masked ? mask_bf16_fails_ : bf16_fails_).load(std::memory_order_relaxed));
        },
        [&] { return (masked ? mask_bf16_window_ : auto_window_).want(); });
}

bool GpuFlatIndex::i8_first(uint64_t n, bool masked) const
{
    const int mode = single_filter_.load(std::memory_order_relaxed);
    const bool ok = !(mode == FILTER_AUTO && i8_unavailable_.load(std::memory_order_relaxed));
    return ladder_stage(
        FILTER_I8, mode, ok, n * (uint64_t)ld_ * sizeof(float), i8_min_bytes_,
        [&] {
            return forced_stage_on((masked ? mask_i8_tries_ : i8_tries_).load(std::memory_order_relaxed),
                                   (masked ? mask_i8_fails_ : i8_fails_).load(std::memory_order_relaxed));
        },
        [&] { return (masked ? mask_i8_window_ : i8_window_).want(); });
}

void GpuFlatIndex::i8_outcome(bool certified, bool masked) const
{
    (masked ? mask_i8_tries_ : i8_tries_).fetch_add(1, std::memory_order_relaxed);
    if (!certified) (masked ? mask_i8_fails_ : i8_fails_).fetch_add(1, std::memory_order_relaxed);
    (masked ? mask_i8_window_ : i8_window_).record(certified);
}

void GpuFlatIndex::bf16_outcome(bool certified, bool masked) const
{
    (masked ? mask_bf16_tries_ : bf16_tries_).fetch_add(1, std::memory_order_relaxed);
    if (!certified) (masked ? mask_bf16_fails_ : bf16_fails_).fetch_add(1, std::memory_order_relaxed);
    (masked ? mask_bf16_window_ : auto_window_).record(certified);
}

int GpuFlatIndex::search_locked(Workspace* ws, const double* query, uint64_t k_eff, int metric,
                                uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n,
                                bool skip_fast, bool skip_bf16, const MmrReq* mmr, const IdFilter* mask) const
{
    const uint64_t n = ids_.size();
    hipStream_t st = ws->stream;
    // Under a mask every stage streams all n rows and drops the excluded ones at the sink: its lists hold kept rows only,
    // so the finalize's bound check and its "a list of every row" rule are about the mask's m rows (search_subset's
    // argument), and a profiled stage read the keep bitmap on top of its rows.
    const bool masked = mask != nullptr;
    const unsigned long long* keep = masked ? mask->d_keep : nullptr;
    const uint64_t n_cert = masked ? mask->m : n;
    const uint64_t keep_bytes = masked ? n / 8 : 0;
    // A diversified search (mmr != nullptr, search_mmr): every stage's finalize leaves its block in DEVICE memory,
    // unstamped, and the selection's two launches behind it write the pinned block and the stamp -- the host waits once,
    // as before, and a stage that did not certify shows in the same flags.
    SearchResultBlock* const fin_out = mmr ? ws->d_result : ws->h_result;
    auto mmr_from_blocks = [&](uint32_t seq) -> int {
        if (!mmr) return OK;
        MmrSource src;
        src.blocks = ws->d_result;
        src.n = (uint32_t)k_eff;
        src.n_block0 = (uint32_t)k_eff;
        return mmr_tail(ws, metric, *mmr, src, seq);
    };
    const uint64_t n_answer = mmr ? mmr->k_out : k_eff;  // what a certified block's n_out says

    const bool q_in_domain = stage_single_query(ws, query, dim_).in_domain;
    // The f32 scan takes its query in the kernel arguments and the finalize kernel reads the pinned block itself,
    // so the common case needs NO copy in front of the kernels.  Every other kernel (bf16 filter, the k > 60 lists,
    // the exact scan: all workgroups read the query) wants it in device memory: copied on first use.
    bool q_on_device = false;
    auto q_to_device = [&]() -> int {
        if (!q_on_device) {
            VL_HIP(hipMemcpyAsync(ws->d_q64, ws->h_q64, (dim_ + 1) * sizeof(double), hipMemcpyHostToDevice, st));
            q_on_device = true;
        }
        return OK;
    };

    const int forced = force_path_.load();
    const bool fast_ok = !skip_fast && forced == 0 && k_eff <= (uint64_t)KFAST_MAX && n_out_of_domain_ == 0 &&
                         q_in_domain;

    // A certified answer of a filter stage: the result block's positions -> the caller's arrays.
    auto take_result = [&](const char* what) -> int {
        if (mmr) {
            set_last_path(PATH_FAST);
            return mmr_take(ws, *mmr, out_pos, out_ids, out_scores, out_n);
        }
        VL_TRY(deliver(what, ids_, ws->h_result, k_eff, out_pos, out_ids, out_scores));
        *out_n = k_eff;
        set_last_path(PATH_FAST);
        return OK;
    };

    // First stage on the largest indexes (auto) or on request (mode 3): scan the int8 copy (a quarter of the f32 slab's
    // bytes).  Its keys bound the score from above, so the same exact f64 rescoring and bound check (with the int8 key's
    // evaluation term) certify the answer or hand the query on: to the bf16 stage when that one is on, else to the f32
    // scan.  Same protocol as below: the query in the kernel arguments, the finalize reading the pinned f64 query.
    bool i8_stage = fast_ok && !skip_bf16 && scan_i8_supported((uint32_t)dim_, metric) && i8_first(n, masked);
    if (i8_stage) {
        const int irc = ensure_i8_slab();
        if (irc != OK) {
            if (single_filter_.load() != FILTER_AUTO) return irc;
            i8_unavailable_.store(true);  // auto: no room for the copy, the next stage answers
            i8_stage = false;
        }
    }
    if (i8_stage) {
        const bool prof = profile_.load();
        const uint32_t ldb = mfma_ldb((uint32_t)dim_);
        I8Query q8;
        prepare_i8_query(query, (uint32_t)dim_, &q8);
        const uint32_t seq = next_stamp(ws);
        int grid = 0, variant = 0;
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        if (masked)
            VL_HIP(launch_scan_i8_masked(st, metric, d_slab8_, d_sr8_, d_norm8_, keep, q8, n, (uint32_t)dim_, ws->d_partials, &grid,
                                         &variant));
        else
            VL_HIP(launch_scan_i8(st, metric, d_slab8_, d_sr8_, d_norm8_, q8, n, (uint32_t)dim_, ws->d_partials, &grid, &variant));
        if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
        // the keys are upper bounds up to their f32 evaluation (mfma_scan.hpp)
        VL_HIP(launch_merge_finalize(st, mmr ? 0u : seq, metric, ws->d_partials, grid, d_master_, ws->h_q64, ws->h_q64 + dim_,
                                     (uint32_t)dim_, n_cert, (uint32_t)k_eff, max_row_norm_, fin_out, IN_EXTRA_I8_SINGLE));
        VL_TRY(mmr_from_blocks(seq));
        note_scan(variant, grid, true);
        VL_TRY(wait_result(ws, seq));
        // the rows plus the per-row (s, r) pair, and |row| for dot
        if (prof)
            VL_TRY(account_profile(ws, n * ((uint64_t)ldb + 2 * sizeof(float) + (metric == DOT ? sizeof(float) : 0)) + keep_bytes));
        const SearchResultBlock& r = *ws->h_result;
        const bool certified = !(r.flags & RESULT_NEEDS_EXACT) && r.n_out == n_answer;
        i8_outcome(certified, masked);
        if (certified) return take_result("int8 filter");
    }

    // Next stage on large indexes (auto) or on request (mode 1): scan the bf16 copy of the slab (half the HBM bytes).
    // Its candidates get the same exact f64 rescoring and a bound with the bf16 row-rounding term; if that cannot
    // certify the answer the f32 scan below runs as before.  Same protocol as the f32 scan: the f32 query in the kernel
    // arguments, the finalize reading the pinned f64 query, a stamped result block -- nothing is copied to the device.
    bool bf16_stage = fast_ok && !skip_bf16 && scan_bf16_supported((uint32_t)dim_, metric) && bf16_first(n, masked);
    if (bf16_stage) {
        const int brc = ensure_bf16_slab(false);
        if (brc != OK) {
            if (single_filter_.load() != FILTER_AUTO) return brc;
            auto_unavailable_.store(true);  // auto: no room for the copy, the f32 path answers
            bf16_stage = false;
        }
    }
    if (bf16_stage) {
        const bool prof = profile_.load();
        const uint32_t ldb = mfma_ldb((uint32_t)dim_);
        const float* q32 = stage_q32(ws, query, dim_, ldb);  // (nearest even is the kernel's own rounding too)
        const uint32_t seq = next_stamp(ws);
        int grid = 0, variant = 0;
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        if (masked)
            VL_HIP(launch_scan_bf16_masked(st, metric, d_slab16_, d_norm16_, d_sqnorm_, keep, n, (uint32_t)dim_, ws->d_partials,
                                           &grid, q32, &variant));
        else
            VL_HIP(launch_scan_bf16(st, metric, d_slab16_, d_norm16_, d_sqnorm_, nullptr, n, (uint32_t)dim_, ws->d_partials,
                                    &grid, q32, &variant));
        if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
        // rows are rounded to bf16, the query is f32 (mfma_scan.hpp)
        VL_HIP(launch_merge_finalize(st, mmr ? 0u : seq, metric, ws->d_partials, grid, d_master_, ws->h_q64, ws->h_q64 + dim_,
                                     (uint32_t)dim_, n_cert, (uint32_t)k_eff, max_row_norm_, fin_out, IN_EXTRA_BF16_SINGLE));
        VL_TRY(mmr_from_blocks(seq));
        note_scan(variant, grid, true);
        VL_TRY(wait_result(ws, seq));
        if (prof) VL_TRY(account_profile(ws, n * (uint64_t)ldb * 2 + keep_bytes));
        const SearchResultBlock& r = *ws->h_result;
        const bool certified = !(r.flags & RESULT_NEEDS_EXACT) && r.n_out == n_answer;
        bf16_outcome(certified, masked);
        if (certified) return take_result("bf16 filter");
    }
    if (fast_ok) {
        const bool prof = profile_.load();
        ScanPlan plan;
        // one search = two launches: the scan (query in its kernel arguments) and the finalize kernel, which reads
        // the f64 query from the pinned block, writes the result block into pinned memory and stamps it; the host
        // waits for the stamp, not for the stream
        const bool qarg = scan_takes_qarg(ld_);
        const float* q32 = qarg ? stage_q32(ws, query, dim_, ld_) : nullptr;
        if (!qarg) VL_TRY(q_to_device());
        const double* fq = q_on_device ? ws->d_q64 : ws->h_q64;
        const uint32_t seq = next_stamp(ws);
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        if (masked)
            VL_HIP(launch_scan_masked(st, metric, d_slab_, d_inv_norm_, keep, n, ws->d_q64, (uint32_t)dim_, ld_, ws->d_partials, &plan, q32));
        else
            VL_HIP(launch_scan(st, metric, d_slab_, d_inv_norm_, ws->d_q64, n, (uint32_t)dim_, ld_, ws->d_partials, &plan, q32));
        if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
        VL_HIP(launch_merge_finalize(st, metric, ws->d_partials, plan.grid, 1, d_master_, fq, fq + dim_, (uint32_t)dim_, n_cert,
                                     (uint32_t)k_eff, max_row_norm_, fin_out, 0.0, mmr ? 0u : seq));
        VL_TRY(mmr_from_blocks(seq));
        note_scan(plan.variant, plan.grid, qarg);
        VL_TRY(wait_result(ws, seq));
        if (prof) VL_TRY(account_profile(ws, n * (uint64_t)ld_ * sizeof(float) + keep_bytes));
        const SearchResultBlock& r = *ws->h_result;
        if (!(r.flags & RESULT_NEEDS_EXACT) && r.n_out == n_answer) return take_result("fast path");
        // ties at the cut or a failed bound: fall through to the exact kernels
    }
    if (masked) return MASK_UNCERTIFIED;  // the exact kernels want the position list: the caller's route

    // 60 < k <= 220: several 64-entry candidate lists (one per partition of the scan's workgroups) rescored and
    // ranked together; still one f32 scan (2.3 ms at N = 10 M) instead of the exact f64 scan + selection rounds
    if (!skip_fast && forced == 0 && k_eff > (uint64_t)KFAST_MAX && k_eff <= (uint64_t)KMULTI_MAX && n_out_of_domain_ == 0 &&
        q_in_domain && n > 4 * (uint64_t)KP) {
        int parts = (int)std::min<uint64_t>(4, (k_eff + 36 + KP - 1) / KP);
        ScanPlan plan;
        VL_TRY(q_to_device());
        VL_HIP(launch_scan(st, metric, d_slab_, d_inv_norm_, ws->d_q64, n, (uint32_t)dim_, ld_, ws->d_partials, &plan));
        while (parts < 4 && plan.grid % parts != 0) ++parts;  // partitions are equal runs of workgroup lists
        if (plan.grid % parts == 0 && plan.grid >= parts) {
            VL_HIP(launch_merge_finalize_multi(st, metric, ws->d_partials, plan.grid, parts, d_master_, ws->d_q64,
                                               ws->d_q64 + dim_, (uint32_t)dim_, n, (uint32_t)k_eff, max_row_norm_,
                                               fin_out));
            VL_TRY(mmr_from_blocks(0));
            VL_HIP(hipStreamSynchronize(st));
            const SearchResultBlock& r0 = ws->h_result[0];
            if (!(r0.flags & RESULT_NEEDS_EXACT) && r0.n_out == n_answer) return take_result("multi-list fast path");
        } else {
            VL_HIP(hipStreamSynchronize(st));
        }
    }

    std::vector<uint32_t> pos;
    std::vector<double> scores;
    VL_TRY(q_to_device());
    VL_TRY(run_exact(ws, metric, n, k_eff, &pos, &scores, nullptr, mmr));
    if (mmr) return mmr_take(ws, *mmr, out_pos, out_ids, out_scores, out_n);
    VL_TRY(deliver("exact path", ids_, pos.data(), scores.data(), k_eff, out_pos, out_ids, out_scores));
    *out_n = k_eff;
    return OK;
}

// Completion of a single search.  The finalize kernel stores the result block in pinned host memory and then the
// stamp (system-scope release); a lone caller polls the stamp -- the block is readable a PCIe write after the kernel's
// last store, where hipStreamSynchronize adds the runtime's own completion path (signal, interrupt or its polling
// interval) on top.  The poll is bounded: the stream is queried now and then so that a failed launch surfaces as an
// error instead of a hang, and when several searches are in flight the threads sleep in hipStreamSynchronize instead
// of each burning a core.
int GpuFlatIndex::wait_result(Workspace* ws, uint32_t seq) const
{
    const uint32_t* stamp = &ws->h_result->seq;
    auto stamped = [&]() { return __atomic_load_n(stamp, __ATOMIC_ACQUIRE) == seq; };
    if (active_searches_.load(std::memory_order_relaxed) <= SPIN_MAX_SEARCHERS) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t it = 1;; ++it) {
            if (stamped()) return OK;
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
            if ((it & 0x3FFF) == 0) {  // every ~16 k polls (some hundred microseconds)
                const hipError_t q = hipStreamQuery(ws->stream);
                if (q == hipSuccess) break;            // stream drained: the stamp is there, or the launch was lost
                if (q != hipErrorNotReady) VL_HIP(q);
                if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(SPIN_MAX_MS)) break;
            }
        }
    }
    VL_HIP(hipStreamSynchronize(ws->stream));
    if (!stamped()) {
        set_last_error("the finalize kernel completed without stamping its result block");
        return ERR_DEVICE;
    }
    return OK;
}

int GpuFlatIndex::run_exact(Workspace* ws, int metric, uint64_t n, uint64_t k_eff, std::vector<uint32_t>* pos,
                            std::vector<double>* scores, const uint32_t* plist, const MmrReq* mmr) const
{
    hipStream_t st = ws->stream;
    // a diversified search: the selection reads the ranked candidates where the kernels below leave them on the device
    // (the rounds' blocks or the sort's arrays; subset indices mapped through plist there) and writes the pinned blocks
    auto mmr_behind = [&](MmrSource src) -> int {
        src.nan_flag = ws->d_nan;
        src.plist = plist;
        src.plist_len = plist ? (uint32_t)n : 0u;
        src.n = (uint32_t)k_eff;
        return mmr_tail(ws, metric, *mmr, src, 0);
    };
    VL_TRY(ensure_scores(ws, n));
    VL_HIP(hipMemsetAsync(ws->d_nan, 0, sizeof(uint32_t), st));
    if (plist)
        VL_HIP(launch_exact_scan_subset(st, metric, d_master_, ws->d_q64, plist, n, (uint32_t)dim_, ws->d_scores, ws->d_nan));
    else
        VL_HIP(launch_exact_scan(st, metric, d_master_, ws->d_q64, n, (uint32_t)dim_, ws->d_scores, ws->d_nan));
    VL_HIP(hipMemcpyAsync(ws->h_nan, ws->d_nan, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    pos->resize(k_eff);
    scores->resize(k_eff);

    if (n == 1) {  // a 1-element sort never calls the comparator: even a NaN score is returned
        VL_HIP(hipMemcpyAsync(scores->data(), ws->d_scores, sizeof(double), hipMemcpyDeviceToHost, st));
        VL_HIP(hipStreamSynchronize(st));
        (*pos)[0] = 0;
        set_last_path(PATH_EXACT_SELECT);
        return OK;
    }

    const int forced = force_path_.load();
    // k <= 64: one selection pass over scores[]; k <= 1024: rounds of 64, each restricted to the rows ranked
    // behind the previous round's last entry (an 80 MB pass per round at N = 10 M instead of a 10 M-element sort)
    const uint64_t rounds = (k_eff + KP - 1) / KP;
    // measured: a round costs ~70 us at N = 1 M and ~140 us at 10 M, the sort 0.34 ms and 6 ms
    const uint64_t max_rounds = std::min<uint64_t>(SELECT_MAX_ROUNDS, std::max<uint64_t>(2, n / 250000));
    const bool use_select = rounds <= max_rounds && forced != PATH_EXACT_SORT;
    if (use_select) {
        for (uint64_t r = 0; r < rounds; ++r) {
            const uint32_t kr = (uint32_t)std::min<uint64_t>(KP, k_eff - r * KP);
            VL_HIP(launch_exact_select(st, ws->d_scores, n, kr, ws->d_partials64, ws->d_nan, ws->d_result + r,
                                       r ? ws->d_result + (r - 1) : nullptr));
        }
        if (mmr) {
            MmrSource src;
            src.blocks = ws->d_result;
            src.n_block0 = (uint32_t)std::min<uint64_t>(KP, k_eff);
            VL_TRY(mmr_behind(src));
        } else {
            VL_HIP(hipMemcpyAsync(ws->h_result, ws->d_result, rounds * sizeof(SearchResultBlock), hipMemcpyDeviceToHost, st));
        }
        VL_HIP(hipStreamSynchronize(st));
    } else {
        const uint64_t cap = sort_capacity_for(n);
        VL_TRY(grow(HipMem{}, ws->sort_cap, cap, {dev_buf(ws->d_okeys, cap), dev_buf(ws->d_opos, cap)}));
        VL_TRY(ensure_out(ws, k_eff));
        VL_HIP(launch_exact_sort(st, ws->d_scores, n, k_eff, ws->d_okeys, ws->d_opos, ws->d_out_pos,
                                 ws->d_out_scores));
        if (mmr) {
            MmrSource src;
            src.pos = ws->d_out_pos;
            src.scores = ws->d_out_scores;
            VL_TRY(mmr_behind(src));
        } else {
            VL_HIP(hipMemcpyAsync(pos->data(), ws->d_out_pos, k_eff * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            VL_HIP(hipMemcpyAsync(scores->data(), ws->d_out_scores, k_eff * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        VL_HIP(hipStreamSynchronize(st));
    }
    if (*ws->h_nan) {
        // sort_by(|a, b| b.score.partial_cmp(&a.score).unwrap()) panics on a NaN (src/index/flat.rs:116)
        set_last_error("NaN similarity score: the reference panics in partial_cmp().unwrap()");
        return ERR_NAN_SCORE;
    }
    if (mmr) {  // the answer stands in the pinned blocks (mmr_take)
        set_last_path(use_select ? PATH_EXACT_SELECT : PATH_EXACT_SORT);
        return OK;
    }
    if (use_select) {
        for (uint64_t r = 0; r < rounds; ++r) {
            const SearchResultBlock& blk = ws->h_result[r];
            const uint64_t kr = std::min<uint64_t>(KP, k_eff - r * KP);
            if (blk.n_out != kr) {
                set_last_error("exact select returned an unexpected result count");
                return ERR_DEVICE;
            }
            for (uint64_t i = 0; i < kr; ++i) {
                (*pos)[r * KP + i] = blk.pos[i];
                (*scores)[r * KP + i] = blk.score[i];
            }
        }
        set_last_path(PATH_EXACT_SELECT);
    } else {
        set_last_path(PATH_EXACT_SORT);
    }
    return OK;
}

// ---------------------------------------------------------------------------------------------
// Search restricted to an id filter.  The contract: exactly FlatIndex::search (src/index/flat.rs:98-119) on a FlatIndex
// that holds only the rows whose id is in the set, in their storage order.  A filter is resolved on the device into the
// ascending list of qualifying storage positions; the subset scan streams only those rows and hands storage positions to
// the same finalize kernel, whose bound check and "the list must hold every row" rule then refer to the m subset rows.
// ---------------------------------------------------------------------------------------------
IdFilter::~IdFilter()
{
    (void)hipSetDevice(device);
    void* dev[] = {d_ids, d_counts, d_plist, d_keep};
    for (void* p : dev)
        if (p) (void)hipFree(p);
}

namespace {
std::atomic<uint64_t> g_next_filter_token{1};  // process-wide: a token is never 0 and never handed out twice
}  // namespace

int GpuFlatIndex::find_filter(uint64_t token, std::shared_ptr<IdFilter>* out) const
{
    return token_find(filters_mu_, filters_, token, UNKNOWN_FILTER, out);
}

int GpuFlatIndex::filter_create(const uint64_t* ids, uint64_t n_ids, uint64_t* out_token, uint64_t* out_rows, bool exclude)
{
    if (!out_token || (!ids && n_ids)) return ERR_INVALID_ARG;
    *out_token = 0;
    if (n_ids >= 0xFFFFFFFFull) {
        set_last_error("a filter holds fewer than 2^32 ids");
        return ERR_INVALID_ARG;
    }
    auto f = std::make_shared<IdFilter>();
    f->device = device_;
    f->kind = exclude ? FilterKind::Exclude : FilterKind::Include;
    f->ids.assign(ids, ids + n_ids);
    std::sort(f->ids.begin(), f->ids.end());
    f->ids.erase(std::unique(f->ids.begin(), f->ids.end()), f->ids.end());
    VL_HIP(hipSetDevice(device_));
    if (!f->ids.empty()) {
        VL_TRY(dev_alloc(&f->d_ids, f->ids.size()));
        VL_HIP(hipMemcpy(f->d_ids, f->ids.data(), f->ids.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    // (an empty exclusion set still resolves on the device: every row qualifies, and rows come and go)
    if (!f->ids.empty() || exclude) VL_TRY(dev_alloc(&f->d_counts, (size_t)FILTER_COUNTS_MAX + 1));
    uint64_t rows = 0;
    {
        std::shared_lock<RwLock> lk(mu_);
        std::lock_guard<std::mutex> fg(f->mu);
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(resolve_filter(lease.ws, f.get())));
        rows = f->m;
    }
    const uint64_t token = g_next_filter_token.fetch_add(1);
    {
        std::lock_guard<std::mutex> g(filters_mu_);
        filters_[token] = std::move(f);
    }
    *out_token = token;
    if (out_rows) *out_rows = rows;
    return OK;
}

int GpuFlatIndex::filter_destroy(uint64_t token)
{
    std::shared_ptr<IdFilter> f;  // a search still using it holds its own reference: freed when that one ends
    return token_take(filters_mu_, filters_, token, UNKNOWN_FILTER, &f);
}

int GpuFlatIndex::filter_rows(uint64_t token, uint64_t* out_rows) const
{
    if (!out_rows) return ERR_INVALID_ARG;
    std::shared_ptr<IdFilter> f;
    VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk(mu_);
    std::lock_guard<std::mutex> fg(f->mu);
    if (filter_stale(f.get())) {
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(resolve_filter(lease.ws, f.get())));
    }
    *out_rows = f->m;
    return OK;
}

int GpuFlatIndex::filter_positions(uint64_t token, std::shared_ptr<IdFilter>* keep, const uint32_t** d_plist, uint64_t* m) const
{
    if (!keep || !d_plist || !m) return ERR_INVALID_ARG;
    std::shared_ptr<IdFilter> f;
    VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk(mu_);
    std::lock_guard<std::mutex> fg(f->mu);
    if (filter_stale(f.get())) {
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(resolve_filter(lease.ws, f.get())));
    }
    if (!f->plist_built) {
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(ensure_plist(lease.ws, f.get())));
    }
    *d_plist = f->d_plist;
    *m = f->m;
    *keep = std::move(f);
    return OK;
}

// positions p < len() whose ids_[p] is in f->ids -> f->d_plist[0..m), ascending.  Two launches, one 4-byte read-back (m, which
// sizes the list and the scan's grid), one launch; nothing per row crosses PCIe.
// An exclusion filter: the same count with the predicate inverted, then the keep bitmap (k_filter_bits); the list waits for
// ensure_plist.  Its empty id set resolves like any other: nf = 0 never reads the set.
// A predicate filter: resolve_where (its columns, then one pass for bitmap and counts); the list waits likewise.
int GpuFlatIndex::resolve_filter(Workspace* ws, IdFilter* f) const
{
    const uint64_t n = ids_.size();
    f->m = 0;
    f->h_plist_valid = false;
    f->plist_built = !f->lazy_list();
    f->resolved_at = ~0ull;
    if (f->kind == FilterKind::Where) {
        VL_TRY(resolve_where(ws, f));
        f->resolved_at = mutations_;
        return OK;
    }
    if (n != 0 && (!f->ids.empty() || f->kind == FilterKind::Exclude)) {
        hipStream_t st = ws->stream;
        VL_TRY(ensure_device_ids());
        VL_HIP(launch_filter_count(st, d_ids_, n, f->d_ids, f->ids.size(), f->d_counts, f->d_counts + FILTER_COUNTS_MAX, f->kind == FilterKind::Exclude));
        uint32_t m = 0;
        VL_HIP(hipMemcpyAsync(&m, f->d_counts + FILTER_COUNTS_MAX, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipStreamSynchronize(st));
        if (m > n) {
            set_last_error("filter resolution counted more rows than the index holds (kernel bug)");
            return ERR_DEVICE;
        }
        if (f->kind == FilterKind::Exclude) {
            const uint64_t words = (n + 63) / 64;
            VL_TRY(grow(HipMem{}, f->keep_cap, words, {dev_buf(f->d_keep, words)}));
            VL_HIP(launch_filter_bits(st, d_ids_, n, f->d_ids, f->ids.size(), f->d_keep));
            VL_HIP(hipStreamSynchronize(st));
        } else {
            VL_TRY(grow(HipMem{}, f->plist_cap, m, {dev_buf(f->d_plist, m)}));
            if (m) {
                VL_HIP(launch_filter_compact(st, d_ids_, n, f->d_ids, f->ids.size(), f->d_counts, m, f->d_plist));
                VL_HIP(hipStreamSynchronize(st));
            }
        }
        f->m = m;
    }
    f->resolved_at = mutations_;
    return OK;
}

// The position list of an exclusion filter, on the first call that needs one after a resolution: k_filter_compact with the
// inverted predicate, at the offsets the resolution's count left in d_counts.
int GpuFlatIndex::ensure_plist(Workspace* ws, IdFilter* f) const
{
    if (f->plist_built) return OK;
    const uint64_t n = ids_.size(), m = f->m;
    VL_TRY(grow(HipMem{}, f->plist_cap, m, {dev_buf(f->d_plist, m)}));
    if (n != 0 && m != 0) {
        if (f->kind == FilterKind::Where)  // from the keep bitmap, in the predicate path's word-aligned chunks
            VL_HIP(launch_where_compact(ws->stream, n, f->d_keep, f->d_counts, m, f->d_plist));
        else
            VL_HIP(launch_filter_compact(ws->stream, d_ids_, n, f->d_ids, f->ids.size(), f->d_counts, m, f->d_plist, true));
        VL_HIP(hipStreamSynchronize(ws->stream));
    }
    f->plist_built = true;
    return OK;
}

// ---------------------------------------------------------------------------------------------
// Attribute columns and predicate filter tokens.  A column is resolved like a group table
// (k_attr_rows: value_of_row[] and the has-bitmap); a predicate token's resolution reads its columns once (k_where_bits) and
// leaves what an exclusion token's leaves: m, the keep bitmap, chunk offsets, the list on demand (k_where_compact).
// ---------------------------------------------------------------------------------------------
AttrColumn::~AttrColumn()
{
    (void)hipSetDevice(device);
    void* dev[] = {d_ids, d_values, d_value_of_row, d_has, d_rows};
    for (void* p : dev)
        if (p) (void)hipFree(p);
}

int GpuFlatIndex::find_attr(uint64_t token, std::shared_ptr<AttrColumn>* out) const
{
    return token_find(filters_mu_, attrs_, token, UNKNOWN_ATTR, out);
}

int GpuFlatIndex::upload_attr(AttrColumn* c) const
{
    const size_t np = c->plan.ids.size();
    VL_HIP(hipSetDevice(device_));
    VL_TRY(grow(HipMem{}, c->pairs_cap, np, {dev_buf(c->d_ids, np), dev_buf(c->d_values, np)}));
    if (np) {
        VL_HIP(hipMemcpy(c->d_ids, c->plan.ids.data(), np * sizeof(uint64_t), hipMemcpyHostToDevice));
        VL_HIP(hipMemcpy(c->d_values, c->plan.values.data(), np * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    return OK;
}

int GpuFlatIndex::attr_create(AttrPlan&& plan, uint64_t* out_token, uint64_t* out_rows)
{
    if (!out_token || plan.ids.size() != plan.values.size()) return ERR_INVALID_ARG;
    *out_token = 0;
    auto c = std::make_shared<AttrColumn>();
    c->device = device_;
    c->plan = std::move(plan);
    VL_TRY(upload_attr(c.get()));
    VL_TRY(dev_alloc(&c->d_rows, 1));
    uint64_t rows = 0;
    {
        std::shared_lock<RwLock> lk(mu_);
        std::lock_guard<std::mutex> cg(c->mu);
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(resolve_attr(lease.ws, c.get())));
        rows = c->rows;
    }
    const uint64_t token = g_next_filter_token.fetch_add(1);
    {
        std::lock_guard<std::mutex> g(filters_mu_);
        attrs_[token] = std::move(c);
    }
    *out_token = token;
    if (out_rows) *out_rows = rows;
    return OK;
}

// The exclusive index lock: no search holds a resolution of this column, or of a token made from it, while the plan and the
// version move.  The next use of the column or of such a token resolves it again.
int GpuFlatIndex::attr_set(uint64_t attr, const uint64_t* ids, const int64_t* values, uint64_t n)
{
    if ((!ids || !values) && n) return ERR_INVALID_ARG;
    std::shared_ptr<AttrColumn> c;
    VL_TRY(find_attr(attr, &c));
    std::unique_lock<RwLock> lk(mu_);
    std::lock_guard<std::mutex> cg(c->mu);
    AttrPlan merged;
    uint64_t bad = 0;
    const int prc = attr_plan_merge(c->plan, ids, values, n, &merged, &bad);
    if (prc != ATTR_PLAN_OK) {
        set_last_error(prc == ATTR_PLAN_TOO_MANY ? "an attribute column holds fewer than 2^32 - 1 pairs"
                                                 : "attribute column: id " + std::to_string(bad) + " is given two different values");
        return ERR_INVALID_ARG;
    }
    std::swap(c->plan, merged);
    const int rc = upload_attr(c.get());
    if (rc != OK) {  // (the device copy may be gone: the old plan goes back up before the error is reported)
        std::swap(c->plan, merged);
        c->resolved_at = ~0ull;
        (void)upload_attr(c.get());
        return rc;
    }
    ++c->version;
    return OK;
}

int GpuFlatIndex::attr_rows(uint64_t attr, uint64_t* out_rows) const
{
    if (!out_rows) return ERR_INVALID_ARG;
    std::shared_ptr<AttrColumn> c;
    VL_TRY(find_attr(attr, &c));
    std::shared_lock<RwLock> lk(mu_);
    std::lock_guard<std::mutex> cg(c->mu);
    if (c->resolved_at != mutations_ || c->resolved_version != c->version) {
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(resolve_attr(lease.ws, c.get())));
    }
    *out_rows = c->rows;
    return OK;
}

int GpuFlatIndex::attr_destroy(uint64_t attr)
{
    std::shared_ptr<AttrColumn> c;  // tokens made from it hold their own references: freed when the last of them goes
    return token_take(filters_mu_, attrs_, attr, UNKNOWN_ATTR, &c);
}

int GpuFlatIndex::resolve_attr(Workspace* ws, AttrColumn* c) const
{
    const uint64_t n = ids_.size();
    c->rows = 0;
    c->resolved_at = ~0ull;
    if (n != 0) {
        hipStream_t st = ws->stream;
        const uint64_t words = (n + 63) / 64;
        VL_TRY(ensure_device_ids());
        VL_TRY(grow(HipMem{}, c->rows_cap, n, {dev_buf(c->d_value_of_row, n)}));
        VL_TRY(grow(HipMem{}, c->has_cap, words, {dev_buf(c->d_has, words)}));
        VL_HIP(launch_attr_rows(st, d_ids_, n, c->d_ids, c->d_values, c->plan.ids.size(), c->d_value_of_row, c->d_has, c->d_rows));
        uint32_t rows = 0;
        VL_HIP(hipMemcpyAsync(&rows, c->d_rows, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipStreamSynchronize(st));
        if (rows > n) {
            set_last_error("column resolution counted more rows than the index holds (kernel bug)");
            return ERR_DEVICE;
        }
        c->rows = rows;
    }
    c->resolved_at = mutations_;
    c->resolved_version = c->version;
    last_where_[3].fetch_add(1, std::memory_order_relaxed);
    return OK;
}

int GpuFlatIndex::filter_create_where(const WhereSpec* clauses, uint64_t n_clauses, uint64_t* out_token, uint64_t* out_rows)
{
    if (!out_token) return ERR_INVALID_ARG;
    *out_token = 0;
    if (n_clauses < 1 || n_clauses > WHERE_MAX_CLAUSES) {
        set_last_error("a predicate filter takes 1 to 4 clauses");
        return ERR_INVALID_ARG;
    }
    if (!clauses) return ERR_INVALID_ARG;
    auto f = std::make_shared<IdFilter>();
    f->device = device_;
    f->kind = FilterKind::Where;
    for (uint64_t i = 0; i < n_clauses; ++i) {
        std::shared_ptr<AttrColumn> c;
        VL_TRY(find_attr(clauses[i].attr, &c));
        f->clauses.push_back({std::move(c), clauses[i].lo, clauses[i].hi, clauses[i].negate, 0});
    }
    VL_HIP(hipSetDevice(device_));
    VL_TRY(dev_alloc(&f->d_counts, (size_t)FILTER_COUNTS_MAX + 1));
    uint64_t rows = 0;
    {
        std::shared_lock<RwLock> lk(mu_);
        std::lock_guard<std::mutex> fg(f->mu);
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(resolve_filter(lease.ws, f.get())));
        rows = f->m;
    }
    const uint64_t token = g_next_filter_token.fetch_add(1);
    {
        std::lock_guard<std::mutex> g(filters_mu_);
        filters_[token] = std::move(f);
    }
    *out_token = token;
    if (out_rows) *out_rows = rows;
    return OK;
}

bool GpuFlatIndex::filter_stale(const IdFilter* f) const
{
    if (f->resolved_at != mutations_) return true;
    for (const WhereClause& cl : f->clauses)
        if (cl.version != cl.column->version) return true;  // (versions move under the exclusive index lock only)
    return false;
}

// The stale columns first, then the predicate: one pass that writes the keep bitmap and the per-chunk counts together, the
// scan that turns them into offsets and m, one 4-byte read-back.
int GpuFlatIndex::resolve_where(Workspace* ws, IdFilter* f) const
{
    const uint64_t n = ids_.size();
    WhereClausesDev dev{};
    dev.n_clauses = (uint32_t)f->clauses.size();
    for (size_t i = 0; i < f->clauses.size(); ++i) {
        WhereClause& cl = f->clauses[i];
        AttrColumn* c = cl.column.get();
        std::lock_guard<std::mutex> cg(c->mu);
        if (c->resolved_at != mutations_ || c->resolved_version != c->version) VL_TRY(resolve_attr(ws, c));
        cl.version = c->version;
        dev.value_of_row[i] = c->d_value_of_row;
        dev.has[i] = c->d_has;
        dev.lo[i] = cl.lo;
        dev.hi[i] = cl.hi;
        dev.negate[i] = cl.negate ? 1u : 0u;
    }
    if (n != 0) {
        hipStream_t st = ws->stream;
        const uint64_t words = (n + 63) / 64;
        VL_TRY(grow(HipMem{}, f->keep_cap, words, {dev_buf(f->d_keep, words)}));
        VL_HIP(launch_where_bits(st, n, dev, f->d_keep, f->d_counts, f->d_counts + FILTER_COUNTS_MAX));
        uint32_t m = 0;
        VL_HIP(hipMemcpyAsync(&m, f->d_counts + FILTER_COUNTS_MAX, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipStreamSynchronize(st));
        if (m > n) {
            set_last_error("predicate resolution counted more rows than the index holds (kernel bug)");
            return ERR_DEVICE;
        }
        f->m = m;
    }
    last_where_[2].fetch_add(1, std::memory_order_relaxed);
    return OK;
}

int GpuFlatIndex::where_first_stage(uint64_t n, int metric) const
{
    // search_locked's ladder under a mask, asked without spending a probe of a paused stage's window
    const int mode = single_filter_.load(std::memory_order_relaxed);
    const uint64_t slab = n * (uint64_t)ld_ * sizeof(float);
    const bool i8 = ladder_stage(
        FILTER_I8, mode, scan_i8_supported((uint32_t)dim_, metric) && !(mode == FILTER_AUTO && i8_unavailable_.load(std::memory_order_relaxed)),
        slab, i8_min_bytes_,
        [&] { return forced_stage_on(mask_i8_tries_.load(std::memory_order_relaxed), mask_i8_fails_.load(std::memory_order_relaxed)); },
        [&] { return mask_i8_window_.on(); });
    if (i8) return WHERE_STAGE_I8;
    const bool bf16 = ladder_stage(
        FILTER_BF16, mode,
        scan_bf16_supported((uint32_t)dim_, metric) && !(mode == FILTER_AUTO && auto_unavailable_.load(std::memory_order_relaxed)), slab,
        auto_min_bytes_,
        [&] { return forced_stage_on(mask_bf16_tries_.load(std::memory_order_relaxed), mask_bf16_fails_.load(std::memory_order_relaxed)); },
        [&] { return mask_bf16_window_.on(); });
    return bf16 ? WHERE_STAGE_BF16 : WHERE_STAGE_F32;
}

int GpuFlatIndex::search_filtered(uint64_t token, const double* query, uint64_t q_len, uint64_t k, int metric,
                                  uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    if (!out_n) return ERR_INVALID_ARG;
    *out_n = 0;
    std::shared_ptr<IdFilter> f;
    VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk;
    VL_TRY(lock_for_query(metric, q_len, &lk));  // the whole index's length check, even when the subset is empty
    if (ids_.empty() || k == 0) return OK;
    if ((!query && dim_) || !out_scores) return ERR_INVALID_ARG;
    // An exclusion filter leaves almost every row in play: where the single-query ladder's conditions hold (and the f32
    // stride is one the masked scan is compiled for) it runs that ladder under the keep bitmap and needs no list.
    // A predicate filter may keep any share of the rows: where_plan.hpp weighs the ladder's first stage against the list.
    const bool ladder = f->has_keep() && force_path_.load() == 0 && n_out_of_domain_ == 0 && scan_masked_supported(ld_);
    const bool where = f->kind == FilterKind::Where;
    return run_search(nullptr, f.get(), [&](Workspace* ws) -> int {
        bool take_ladder = ladder;
        if (where) {
            const WhereShape shp{ladder, ids_.size(), ld_, mfma_ldb((uint32_t)dim_), where_first_stage(ids_.size(), metric),
                                 (uint64_t)KFAST_MAX};
            take_ladder = where_route_mask(where_route_.load(), shp, f->m, k);
            last_where_[0].store(take_ladder ? 1 : 0, std::memory_order_relaxed);
            last_where_[1].store(f->m, std::memory_order_relaxed);
        }
        if (f->m == 0) return OK;
        const uint64_t k_eff = std::min<uint64_t>(k, f->m);
        bool uncertified = false;
        if (take_ladder && k_eff <= (uint64_t)KFAST_MAX) {
            const int rc = search_locked(ws, query, k_eff, metric, out_pos, out_ids, out_scores, out_n, false, false, nullptr, f.get());
            if (rc != MASK_UNCERTIFIED) return rc;
            uncertified = true;  // no masked stage certified it (or the query is out of the domain): the exact kernels
        }
        if (f->lazy_list()) {
            std::lock_guard<std::mutex> fg(f->mu);
            VL_TRY(ensure_plist(ws, f.get()));
        }
        return search_subset(ws, f.get(), query, k_eff, metric, out_pos, out_ids, out_scores, out_n, nullptr, uncertified);
    }, /*need_list=*/!f->lazy_list());
}

int GpuFlatIndex::search_subset(Workspace* ws, IdFilter* f, const double* query, uint64_t k_eff, int metric,
                                uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n,
                                const MmrReq* mmr, bool exact_only) const
{
    const uint64_t m = f->m;
    const uint32_t* plist = f->d_plist;
    hipStream_t st = ws->stream;
    const uint64_t n_answer = mmr ? mmr->k_out : k_eff;  // (search_locked's protocol for a diversified search)

    const bool q_in_domain = stage_single_query(ws, query, dim_).in_domain;
    bool q_on_device = false;
    auto q_to_device = [&]() -> int {
        if (!q_on_device) {
            VL_HIP(hipMemcpyAsync(ws->d_q64, ws->h_q64, (dim_ + 1) * sizeof(double), hipMemcpyHostToDevice, st));
            q_on_device = true;
        }
        return OK;
    };

    // the fast path's conditions are search_locked's; the out-of-domain count is the whole index's (conservative)
    const bool fast_ok = !exact_only && force_path_.load() == 0 && k_eff <= (uint64_t)KFAST_MAX && n_out_of_domain_ == 0 && q_in_domain;
    if (fast_ok) {
        const bool prof = profile_.load();
        ScanPlan plan;
        const bool qarg = scan_subset_takes_qarg(ld_);
        const float* q32 = qarg ? stage_q32(ws, query, dim_, ld_) : nullptr;
        if (!qarg) VL_TRY(q_to_device());
        const double* fq = q_on_device ? ws->d_q64 : ws->h_q64;
        const uint32_t seq = next_stamp(ws);
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        VL_HIP(launch_scan_subset(st, metric, d_slab_, d_inv_norm_, plist, m, ws->d_q64, (uint32_t)dim_, ld_, ws->d_partials,
                                  &plan, q32));
        if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
        // n_rows = m: the bound check and the "a list of every row" rule are about the subset (every row left out of the
        // lists is a subset row with a key at or below the 64th; rows outside the subset are no part of the answer)
        VL_HIP(launch_merge_finalize(st, metric, ws->d_partials, plan.grid, 1, d_master_, fq, fq + dim_, (uint32_t)dim_, m,
                                     (uint32_t)k_eff, max_row_norm_, mmr ? ws->d_result : ws->h_result, 0.0, mmr ? 0u : seq));
        if (mmr) {
            MmrSource src;
            src.blocks = ws->d_result;
            src.n = (uint32_t)k_eff;
            src.n_block0 = (uint32_t)k_eff;
            VL_TRY(mmr_tail(ws, metric, *mmr, src, seq));
        }
        note_scan(plan.variant, plan.grid, qarg);
        VL_TRY(wait_result(ws, seq));
        // the rows read, the position list, and 1/|row| for cosine
        if (prof) VL_TRY(account_profile(ws, m * ((uint64_t)ld_ * sizeof(float) + sizeof(uint32_t) + (metric == COSINE ? sizeof(float) : 0))));
        const SearchResultBlock& r = *ws->h_result;
        if (!(r.flags & RESULT_NEEDS_EXACT) && r.n_out == n_answer) {
            if (mmr) {
                set_last_path(PATH_FAST);
                return mmr_take(ws, *mmr, out_pos, out_ids, out_scores, out_n);
            }
            VL_TRY(deliver("filtered fast path", ids_, &r, k_eff, out_pos, out_ids, out_scores));
            *out_n = k_eff;
            set_last_path(PATH_FAST);
            return OK;
        }
        // ties at the cut or a failed bound: the exact kernels over the subset
    }

    std::vector<uint32_t> idx;
    std::vector<double> scores;
    VL_TRY(q_to_device());
    VL_TRY(run_exact(ws, metric, m, k_eff, &idx, &scores, plist, mmr));
    if (mmr) return mmr_take(ws, *mmr, out_pos, out_ids, out_scores, out_n);  // storage positions already
    {
        std::lock_guard<std::mutex> fg(f->mu);
        if (!f->h_plist_valid) {  // one copy of the list per resolution, on the first exact answer that needs it
            f->h_plist.resize(m);
            VL_HIP(hipMemcpyAsync(f->h_plist.data(), plist, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            VL_HIP(hipStreamSynchronize(st));
            f->h_plist_valid = true;
        }
    }
    auto storage_pos = [&](uint64_t i) { return idx[i] < m ? f->h_plist[idx[i]] : POS_SENTINEL; };
    VL_TRY(deliver("filtered exact path", ids_, k_eff, storage_pos, [&](uint64_t i) { return scores[i]; }, out_pos, out_ids, out_scores));
    *out_n = k_eff;
    return OK;
}

// A batch of filtered searches, one filter for all queries or one per query.  Every (query, filter)
// pair is a job.  The jobs that may take the fast path are planned into launches (subset_batch_plan.hpp); a launch is one
// H2D copy of its queries, norms and job table, one k_scan_subset_jobs, one finalize into the pinned K3 result blocks and
// one stream sync -- search_batch's K3 pipeline, where the single path pays a launch pair and a stamp wait per query.
// The certificate is the single path's, per job (n_rows = m, k = min(k, m)); what it refuses goes to the exact kernels,
// what the plan left out to search_subset.
static_assert(sizeof(SubsetJobDev) == 2 * sizeof(double), "k3_stage_words() counts two words per job table entry");

int GpuFlatIndex::search_batch_filters(const uint64_t* tokens, uint64_t n_filters, const double* queries, uint64_t nq,
                                       uint64_t q_len, uint64_t k, int metric, uint64_t out_stride, uint64_t* out_ids,
                                       double* out_scores, uint64_t* out_n) const
{
    if (nq == 0) return OK;
    if (!out_n) return ERR_INVALID_ARG;
    for (uint64_t i = 0; i < nq; ++i) out_n[i] = 0;
    if (n_filters != 1 && n_filters != nq) {
        set_last_error("a filtered batch takes one filter, or one filter per query");
        return ERR_INVALID_ARG;
    }
    if (!tokens) return ERR_INVALID_ARG;
    // every distinct token is looked up once; the references keep the filters alive until the call ends
    std::vector<std::shared_ptr<IdFilter>> filters;
    std::vector<uint32_t> filter_of(n_filters);
    {
        std::unordered_map<uint64_t, uint32_t> slot;
        for (uint64_t i = 0; i < n_filters; ++i) {
            auto it = slot.find(tokens[i]);
            if (it == slot.end()) {
                std::shared_ptr<IdFilter> f;
                VL_TRY(find_filter(tokens[i], &f));
                it = slot.emplace(tokens[i], (uint32_t)filters.size()).first;
                filters.push_back(std::move(f));
            }
            filter_of[i] = it->second;
        }
    }
    std::shared_lock<RwLock> lk;
    VL_TRY(lock_for_query(metric, q_len, &lk));  // the whole index's length check, even when every subset is empty
    if (ids_.empty() || k == 0) return OK;
    if ((!queries && dim_) || !out_ids || !out_scores || k > out_stride) return ERR_INVALID_ARG;

    WsLease lease(this, /*sync_always=*/true);
    if (lease.status() != OK) return lease.status();
    Workspace* const ws = lease.ws;
    hipStream_t st = ws->stream;
    // each stale filter once, whatever its number of jobs; an exclusion token's position list waits until one of its
    // queries needs it (need_list below): the masked MFMA pass reads the keep bitmap
    for (const auto& f : filters) VL_TRY(resolve_if_stale(ws, f.get(), /*need_list=*/!f->lazy_list()));
    InFlight searching(active_searches_);

    auto filter_at = [&](uint64_t qi) { return filters[filter_of[n_filters == 1 ? 0 : qi]].get(); };
    const bool may_batch = force_path_.load() == 0 && n_out_of_domain_ == 0 && dim_ != 0;
    uint64_t mb[5] = {0, 0, 0, 0, 0};  // last_masked_batch: routed, certified, handed back, sequences, lists built
    auto publish_masked = [&]() {
        for (int i = 0; i < 5; ++i) last_mbatch_[i].store(mb[i], std::memory_order_relaxed);
    };
    auto need_list = [&](IdFilter* f) -> int {
        std::lock_guard<std::mutex> g(f->mu);
        if (f->plist_built) return OK;
        ++mb[4];
        return ensure_plist(ws, f);
    };

    // ---- exclusion tokens: the mask-aware MFMA pass answers the eligible queries it may take
    //      (masked_batch_plan.hpp); what it does not certify joins the jobs below like any other query ----
    std::vector<uint8_t> answered(nq, 0);
    {
        const uint64_t n = ids_.size();
        const char* mf_env = getenv("VL_MFMA");
        const char* mf_min = getenv("VL_MFMA_MIN_BATCH");
        const MaskedBatchShape shp{may_batch && !(mf_env && mf_env[0] == '0') && mfma_scan_supported((uint32_t)dim_, metric) &&
                                       mfma_rows_kernel((uint32_t)dim_),
                                   n, (uint32_t)dim_, ld_, mfma_ldb((uint32_t)dim_)};
        const MaskedBatchLimits lim{MFMA_MIN_ROWS, mf_min && *mf_min ? (uint64_t)atoi(mf_min) : (uint64_t)MFMA_MIN_BATCH,
                                    (uint64_t)KFAST_MAX, mfma_sequence_queries((uint32_t)dim_)};
        const int mode = masked_batch_.load();
        std::vector<uint32_t> elig;
        uint64_t sum_m = 0;
        if (mode != MASKED_BATCH_OFF && shp.index_ok)
            for (uint64_t qi = 0; qi < nq; ++qi) {
                const IdFilter* f = filter_at(qi);
                if (f->has_keep() && masked_query_eligible(shp, lim, f->m, k)) {
                    elig.push_back((uint32_t)qi);
                    sum_m += f->m;
                }
            }
        if (masked_batch_route(mode, shp, lim, elig.size(), sum_m)) {
            const uint64_t ne = elig.size();
            std::vector<const unsigned long long*> keep(ne);
            std::vector<uint32_t> mq(ne), kq(ne);
            for (uint64_t j = 0; j < ne; ++j) {
                const IdFilter* f = filter_at(elig[j]);
                keep[j] = f->d_keep;
                mq[j] = (uint32_t)f->m;
                kq[j] = (uint32_t)std::min<uint64_t>(k, f->m);
            }
            const MaskedQueries desc{elig.data(), keep.data(), mq.data(), kq.data()};
            std::vector<uint64_t> t_ids(ne * k), t_n(ne, 0);
            std::vector<double> t_scores(ne * k);
            std::vector<uint8_t> done(ne, 0);
            const int rc = search_batch_mfma(ws, queries, nullptr, ne, k, k, metric, nullptr, t_ids.data(), t_scores.data(), t_n.data(),
                                             &done, nullptr, &desc, &mb[3]);
            if (rc != OK) {
                publish_masked();
                return rc;
            }
            mb[0] = ne;
            for (uint64_t j = 0; j < ne; ++j) {
                if (!done[j]) continue;
                const uint64_t qi = elig[j];
                std::copy_n(t_ids.data() + j * k, t_n[j], out_ids + qi * out_stride);
                std::copy_n(t_scores.data() + j * k, t_n[j], out_scores + qi * out_stride);
                out_n[qi] = t_n[j];
                answered[qi] = 1;
                ++mb[1];
            }
            mb[2] = mb[0] - mb[1];
            if (mb[1]) set_last_path(PATH_FAST);
        }
    }
    // the position lists the jobs kernel and search_subset read: every token with a query left (one that keeps no row
    // is answered empty without a list)
    for (uint64_t qi = 0; qi < nq; ++qi)
        if (!answered[qi] && filter_at(qi)->lazy_list() && filter_at(qi)->m > 0) {
            const int rc = need_list(filter_at(qi));
            if (rc != OK) {
                publish_masked();
                for (uint64_t q = 0; q < nq; ++q) out_n[q] = 0;
                return rc;
            }
        }
    publish_masked();
    int shape_g = 1, shape_u = 1, resident = 1;
    if (may_batch) VL_HIP(scan_subset_jobs_shape(metric, ld_, &shape_g, &shape_u, &resident));
    std::vector<SubsetJob> jobs(nq);
    for (uint64_t qi = 0; qi < nq; ++qi) {
        const uint64_t m = answered[qi] ? 0 : filter_at(qi)->m;  // (m = 0: the plan leaves the query alone)
        jobs[qi].m = m;
        jobs[qi].need = subset_job_need(m, shape_g, shape_u);
        jobs[qi].fast = may_batch && m > 0 && std::min<uint64_t>(k, m) <= (uint64_t)KFAST_MAX && query_in_domain(queries + qi * dim_, dim_);
    }
    const SubsetBatchPlan plan = subset_batch_plan(
        jobs, {(uint32_t)resident, (uint32_t)K3_PIPE_QUERIES, (uint64_t)PARTIALS32_LISTS, (uint32_t)SCAN_BATCH_QB, (uint32_t)SCAN_BATCH_MAX_GRID});

    enum : uint8_t { DONE = 0, SINGLE = 1, EXACT = 2 };  // DONE: answered (an empty subset, or a certified batched job)
    std::vector<uint8_t> todo(nq, DONE);
    for (uint32_t qi : plan.single) todo[qi] = SINGLE;
    uint64_t n_batched = 0, n_exact = 0;

    if (!plan.launches.empty()) {
        const size_t k3_words = k3_stage_words(dim_);
        VL_TRY(ensure_set(HipMem{}, {dev_buf(ws->k3_d_q64, k3_words), pinned_buf(ws->k3_h_q64, k3_words),
                                     pinned_buf(ws->k3_h_result, K3_PIPE_QUERIES)}));
    }
    const bool prof = profile_.load();
    std::vector<uint8_t> in_domain((size_t)K3_PIPE_QUERIES);
    for (const SubsetLaunch& L : plan.launches) {
        const uint32_t cnt = (uint32_t)L.jobs.size();
        // the launch's pinned block: cnt queries, cnt norms, cnt job table entries -- one H2D copy
        double* norms = ws->k3_h_q64 + (size_t)cnt * dim_;
        SubsetJobDev* h_jobs = reinterpret_cast<SubsetJobDev*>(norms + cnt);
        uint64_t bytes = 0;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t qi = L.jobs[j];
            const IdFilter* f = filter_at(qi);
            in_domain[j] = stage_query(queries + qi * dim_, ws->k3_h_q64 + (size_t)j * dim_, dim_, &norms[j]) ? 1 : 0;
            h_jobs[j].plist = f->d_plist;
            h_jobs[j].m = (uint32_t)f->m;
            h_jobs[j].k = (uint32_t)std::min<uint64_t>(k, f->m);
            bytes += f->m * ((uint64_t)ld_ * sizeof(float) + sizeof(uint32_t) + (metric == COSINE ? sizeof(float) : 0));
        }
        VL_HIP(hipMemcpyAsync(ws->k3_d_q64, ws->k3_h_q64, ((size_t)cnt * dim_ + 3 * (size_t)cnt) * sizeof(double), hipMemcpyHostToDevice, st));
        const double* d_norms = ws->k3_d_q64 + (size_t)cnt * dim_;
        const SubsetJobDev* d_jobs = reinterpret_cast<const SubsetJobDev*>(d_norms + cnt);
        ScanPlan sp;
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        VL_HIP(launch_scan_subset_jobs(st, metric, d_slab_, d_inv_norm_, d_jobs, cnt, L.gx, ws->k3_d_q64, (uint32_t)dim_, ld_,
                                       ws->d_partials, &sp));
        if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
        VL_HIP(launch_merge_finalize_jobs(st, metric, ws->d_partials, (int)L.gx, d_jobs, cnt, d_master_, ws->k3_d_q64, d_norms,
                                          (uint32_t)dim_, max_row_norm_, ws->k3_h_result));
        VL_HIP(hipStreamSynchronize(st));
        note_scan(sp.variant, sp.grid, false);
        if (prof) VL_TRY(account_profile(ws, bytes));
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t qi = L.jobs[j];
            const uint64_t k_eff = h_jobs[j].k;
            const SearchResultBlock& r = ws->k3_h_result[j];  // (a fallback below uses the workspace's other buffers, not these)
            if (in_domain[j] && !(r.flags & RESULT_NEEDS_EXACT) && r.n_out == k_eff) {
                VL_TRY(deliver("filtered batch fast path", ids_, &r, k_eff, nullptr, out_ids + qi * out_stride, out_scores + qi * out_stride));
                out_n[qi] = k_eff;
                ++n_batched;
            } else {
                todo[qi] = EXACT;
                ++n_exact;
            }
        }
        set_last_path(PATH_FAST);
    }
    last_fbatch_[0].store(n_batched, std::memory_order_relaxed);
    last_fbatch_[1].store(plan.single.size(), std::memory_order_relaxed);
    last_fbatch_[2].store(n_exact, std::memory_order_relaxed);
    last_fbatch_[3].store(plan.launches.size(), std::memory_order_relaxed);

    // what is left, in query order; the first failure ends the call (rows in front of it keep their answers)
    for (uint64_t qi = 0; qi < nq; ++qi) {
        if (todo[qi] == DONE) continue;
        IdFilter* f = filter_at(qi);
        const int rc = search_subset(ws, f, queries + qi * dim_, std::min<uint64_t>(k, f->m), metric, nullptr, out_ids + qi * out_stride,
                                     out_scores + qi * out_stride, out_n + qi, nullptr, todo[qi] == EXACT);
        if (rc != OK) {
            for (uint64_t q = qi; q < nq; ++q) out_n[q] = 0;
            return rc;
        }
    }
    return OK;
}

// ---------------------------------------------------------------------------------------------
// Diversified search: maximal marginal relevance over the candidates of FlatIndex::search(q, fetch_k)
// (src/index/flat.rs:98-119), on the whole index or on a filter's rows.  The search runs as it always does -- the ladder,
// the multi-list route, the exact kernels -- except that its last kernel leaves the ranked candidates in device memory;
// k_mmr_pairwise and k_mmr_select follow on the same stream and write the chosen (position, score) pairs into the pinned
// result blocks.  Given exact candidates the selection is a deterministic function of reference scores: nothing to certify.
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::mmr_tail(Workspace* ws, int metric, const MmrReq& m, MmrSource src, uint32_t seq) const
{
    src.n_rows = (uint32_t)ids_.size();
    VL_HIP(launch_mmr(ws->stream, metric, d_master_, (uint32_t)dim_, src, ws->mmr_sim, (uint32_t)m.k_out, m.lambda, ws->h_result,
                      seq));
    return OK;
}

int GpuFlatIndex::mmr_take(Workspace* ws, const MmrReq& m, uint64_t* out_pos, uint64_t* out_ids, double* out_scores,
                           uint64_t* out_n) const
{
    if (ws->h_result[0].flags != 0u || ws->h_result[0].n_out != m.k_out) {
        set_last_error("the selection kernel did not take the search's candidates (kernel bug)");
        return ERR_DEVICE;
    }
    VL_TRY(deliver("diversified search", ids_, ws->h_result, m.k_out, out_pos, out_ids, out_scores));
    *out_n = m.k_out;
    return OK;
}

int GpuFlatIndex::search_mmr(uint64_t token, const double* query, uint64_t q_len, uint64_t k, uint64_t fetch_k, double lambda,
                             int metric, uint64_t out_capacity, uint64_t* out_pos, uint64_t* out_ids, double* out_scores,
                             uint64_t* out_n) const
{
    if (!out_n) return ERR_INVALID_ARG;
    *out_n = 0;
    VL_TRY(mmr_check_args(k, fetch_k, lambda));
    std::shared_ptr<IdFilter> f;
    if (token != 0) VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk;  // held from the search to the selection: positions cannot move in between
    VL_TRY(lock_for_query(metric, q_len, &lk));
    const uint64_t n = ids_.size();
    const uint64_t k_cap = std::min<uint64_t>(k, out_capacity);  // a smaller k's answer is a prefix
    if (n == 0 || k_cap == 0) return OK;
    if ((!query && dim_) || !out_scores) return ERR_INVALID_ARG;
    return run_search(nullptr, f.get(), [&](Workspace* ws) -> int {
        return search_mmr_locked(ws, f.get(), query, k_cap, fetch_k, lambda, metric, out_pos, out_ids, out_scores, out_n);
    });
}

int GpuFlatIndex::search_mmr_locked(Workspace* ws, IdFilter* f, const double* query, uint64_t k_cap, uint64_t fetch_k, double lambda,
                                    int metric, uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    const uint64_t rows = f ? f->m : ids_.size();
    if (rows == 0) return OK;
    const uint64_t fetch_eff = std::min<uint64_t>(fetch_k, rows);
    const MmrReq req{std::min<uint64_t>(k_cap, fetch_eff), lambda};
    if (req.k_out == 1) {
        // sel = [0]: the best of search(q, fetch_k), whose errors are this call's
        std::vector<uint64_t> pos(fetch_eff), ids(fetch_eff);
        std::vector<double> scores(fetch_eff);
        uint64_t got = 0;
        VL_TRY(f ? search_subset(ws, f, query, fetch_eff, metric, pos.data(), ids.data(), scores.data(), &got)
                 : search_locked(ws, query, fetch_eff, metric, pos.data(), ids.data(), scores.data(), &got, false));
        if (got >= 1) {
            if (out_pos) out_pos[0] = pos[0];
            if (out_ids) out_ids[0] = ids[0];
            out_scores[0] = scores[0];
            *out_n = 1;
        }
        return OK;
    }
    if (!ws->mmr_sim) VL_TRY(dev_alloc(&ws->mmr_sim, (size_t)MMR_MAX_FETCH * MMR_MAX_FETCH));
    return f ? search_subset(ws, f, query, fetch_eff, metric, out_pos, out_ids, out_scores, out_n, &req)
             : search_locked(ws, query, fetch_eff, metric, out_pos, out_ids, out_scores, out_n, false, false, &req);
}

// ---------------------------------------------------------------------------------------------
// Batched diversified search: nq MMR queries against one index state.  MMR needs the first
// n = min(fetch_k, m) rows of S's ranking, exact and in order, and nothing behind them: the certified prefix of the MFMA
// batch filter's rescored 64-entry list (section 26) gives them whenever it is n long.  k_mmr_batch_rank decides that per
// query, k_mmr_batch_select computes the n candidates' similarities and runs the selection; a query the pass does not
// settle runs the single search's body under the same lock, so each row is the single call's answer bit for bit.
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::search_mmr_batch(uint64_t token, const double* queries, uint64_t nq, uint64_t q_len, uint64_t k, uint64_t fetch_k,
                                   double lambda, int metric, uint64_t out_stride, uint64_t* out_ids, double* out_scores,
                                   uint64_t* out_n) const
{
    uint64_t mb[4] = {0, 0, 0, 0};  // last_mmr_batch: routed, settled, handed back, sequences
    auto publish = [&]() {
        for (int i = 0; i < 4; ++i) last_mmrbatch_[i].store(mb[i], std::memory_order_relaxed);
    };
    if (nq == 0) {
        publish();
        return OK;
    }
    if (!out_n) return ERR_INVALID_ARG;
    for (uint64_t i = 0; i < nq; ++i) out_n[i] = 0;
    set_last_path(PATH_NONE);
    VL_TRY(mmr_check_args(k, fetch_k, lambda));
    std::shared_ptr<IdFilter> f;
    if (token != 0) VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk;  // one index state for the whole batch
    VL_TRY(lock_for_query(metric, q_len, &lk));
    publish();
    const uint64_t n = ids_.size();
    const uint64_t k_cap = std::min<uint64_t>(k, out_stride);  // out_stride is the single call's capacity
    if (n == 0 || k_cap == 0) return OK;
    if ((!queries && dim_) || !out_scores) return ERR_INVALID_ARG;

    WsLease lease(this, /*sync_always=*/true);
    if (lease.status() != OK) return lease.status();
    Workspace* const ws = lease.ws;
    // an exclusion token's position list waits until a query is left to the single search: the pass reads a bitmap
    if (f) VL_TRY(resolve_if_stale(ws, f.get(), /*need_list=*/!f->lazy_list()));
    InFlight searching(active_searches_);
    const uint64_t m = f ? f->m : n;
    if (m == 0) return OK;  // an empty S (search_mmr's early return)

    std::vector<uint8_t> done(nq, 0);
    {
        const char* mf_env = getenv("VL_MFMA");
        const char* mf_min = getenv("VL_MFMA_MIN_BATCH");
        const MaskedBatchLimits lim{MFMA_MIN_ROWS, mf_min && *mf_min ? (uint64_t)atoi(mf_min) : (uint64_t)MFMA_MIN_BATCH,
                                    (uint64_t)KFAST_MAX, mfma_sequence_queries((uint32_t)dim_)};
        MmrBatchShape shp;
        shp.index = {force_path_.load() == 0 && n_out_of_domain_ == 0 && dim_ != 0 && !(mf_env && mf_env[0] == '0') &&
                         mfma_scan_supported((uint32_t)dim_, metric),
                     n, (uint32_t)dim_, ld_, mfma_ldb((uint32_t)dim_)};
        shp.rows_kernel = mfma_rows_kernel((uint32_t)dim_);
        shp.filtered = f != nullptr;
        shp.include = f && !f->has_keep();
        shp.m = m;
        shp.i8_min_bytes = i8_min_bytes_;
        shp.bf16_min_bytes = auto_min_bytes_;
        if (mmr_batch_route(mmr_batch_.load(), shp, lim, nq, fetch_k)) {
            const uint64_t n_need = std::min<uint64_t>(fetch_k, m);
            const unsigned long long* keep = nullptr;
            if (f && f->has_keep()) {
                keep = f->d_keep;  // the token's own bitmap (section 24)
            } else if (f) {        // an include token: its rows as a bitmap, in the borrowed workspace; no list is read
                const uint64_t words = (n + 63) / 64;
                VL_TRY(grow(HipMem{}, ws->gb_keep_cap, words, {dev_buf(ws->gb_keep, words)}));
                VL_TRY(ensure_device_ids());
                VL_HIP(launch_filter_bits(ws->stream, d_ids_, n, f->d_ids, f->ids.size(), ws->gb_keep, /*include=*/true));
                keep = ws->gb_keep;
            }
            std::vector<uint32_t> qidx, mq, kq;
            std::vector<const unsigned long long*> keep_of;
            MaskedQueries desc{nullptr, nullptr, nullptr, nullptr};
            if (keep) {  // every query of every sequence under the ONE bitmap of S
                qidx.resize(nq);
                for (uint64_t i = 0; i < nq; ++i) qidx[i] = (uint32_t)i;
                mq.assign(nq, (uint32_t)m);
                kq.assign(nq, (uint32_t)n_need);
                keep_of.assign(nq, keep);
                desc = {qidx.data(), keep_of.data(), mq.data(), kq.data()};
            }
            const MmrBatchReq req{m, n_need, std::min<uint64_t>(k_cap, n_need), lambda, out_stride};
            VL_TRY(search_batch_mfma(ws, queries, nullptr, nq, out_stride, n_need, metric, nullptr, out_ids, out_scores, out_n, &done,
                                     nullptr, keep ? &desc : nullptr, &mb[3], nullptr, &req));
            mb[0] = nq;
            for (uint64_t qi = 0; qi < nq; ++qi) mb[1] += done[qi] ? 1 : 0;
            mb[2] = mb[0] - mb[1];
        }
    }
    // what the pass did not settle (or everything), in ascending order: the first failure is the lowest failing query
    bool list_ready = !(f && f->lazy_list());
    for (uint64_t qi = 0; qi < nq; ++qi) {
        if (done[qi]) continue;
        if (!list_ready) {
            std::lock_guard<std::mutex> fg(f->mu);
            VL_TRY(ensure_plist(ws, f.get()));
            list_ready = true;
        }
        VL_TRY(search_mmr_locked(ws, f.get(), queries + qi * dim_, k_cap, fetch_k, lambda, metric, nullptr,
                                 out_ids ? out_ids + qi * out_stride : nullptr, out_scores + qi * out_stride, out_n + qi));
    }
    if (mb[1]) set_last_path(PATH_FAST);
    publish();
    return OK;
}

// ---------------------------------------------------------------------------------------------
// Range search: every row whose reference score is >= min_score.  The contract: the longest prefix
// of FlatIndex::search(q, len, metric) (src/index/flat.rs:98-119) -- over the filter's rows when a filter is given -- whose
// scores satisfy score >= min_score.  The threshold becomes a threshold on scan keys through the shipped bound
// (score_bound.hpp): a row whose bound is below min_score is provably out, every other row is rescored in the
// reference's f64 order and cut on that score.  Nothing is left to certify, so the fast route has no "could not certify"
// exit; it leaves for the exact route only when the candidate buffer overflows (or data / query are out of the domain).
// ---------------------------------------------------------------------------------------------
namespace {
uint32_t range_candidate_capacity()
{
    // VL_RANGE_CAND_CAP: a smaller candidate buffer (tests drive the overflow route with it)
    if (const char* e = getenv("VL_RANGE_CAND_CAP")) {
        const long long v = atoll(e);
        if (v >= 1 && v <= (long long)RANGE_CAND_MAX) return (uint32_t)v;
    }
    return RANGE_CAND_MAX;
}
}  // namespace

int GpuFlatIndex::search_range(uint64_t token, const double* query, uint64_t q_len, double min_score, int metric,
                               uint64_t out_capacity, uint64_t* out_pos, uint64_t* out_ids, double* out_scores,
                               uint64_t* out_n, uint64_t* out_total) const
{
    if (!out_n || !out_total) return ERR_INVALID_ARG;
    *out_n = 0;
    *out_total = 0;
    std::shared_ptr<IdFilter> f;
    if (token != 0) VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk;
    VL_TRY(lock_for_query(metric, q_len, &lk));
    if (min_score != min_score) {
        set_last_error("min_score is NaN");
        return ERR_INVALID_ARG;
    }
    if (ids_.empty()) return OK;
    if ((!query && dim_) || (out_capacity != 0 && !out_scores)) return ERR_INVALID_ARG;
    return run_search(nullptr, f.get(), [&](Workspace* ws) -> int {
        if (f && f->m == 0) return OK;
        return search_range_locked(ws, f.get(), query, min_score, metric, out_capacity, out_pos, out_ids, out_scores, out_n, out_total);
    });
}

int GpuFlatIndex::search_range_locked(Workspace* ws, IdFilter* f, const double* query, double min_score, int metric,
                                      uint64_t out_capacity, uint64_t* out_pos, uint64_t* out_ids, double* out_scores,
                                      uint64_t* out_n, uint64_t* out_total) const
{
    const uint64_t n = ids_.size();
    const uint64_t m = f ? f->m : n;               // the rows of "the index" the contract speaks of
    const uint32_t* plist = f ? f->d_plist : nullptr;
    hipStream_t st = ws->stream;

    const StagedQuery sq = stage_single_query(ws, query, dim_);
    VL_HIP(hipMemcpyAsync(ws->d_q64, ws->h_q64, (dim_ + 1) * sizeof(double), hipMemcpyHostToDevice, st));

    // writes the answer's first `want` entries from (positions, scores) on the host
    auto answer = [&](const uint32_t* pos, const double* scores, uint64_t want, uint64_t total) -> int {
        VL_TRY(deliver("range search", ids_, pos, scores, want, out_pos, out_ids, out_scores));
        *out_n = want;
        *out_total = total;
        return OK;
    };

    const uint32_t cap = range_candidate_capacity();
    const bool fast_ok = force_path_.load() == 0 && n_out_of_domain_ == 0 && sq.in_domain;
    if (fast_ok) {
        VL_TRY(ensure_range_ws(ws, RANGE_CAND_MAX, RANGE_SMALL));
        VL_TRY(ensure_range_candidates(ws));
        // the score threshold in key space: rows with key <= tau are provably below min_score (R over the whole index
        // bounds a filter's rows too); no such key: every row is a candidate (NaN fails the device's comparison)
        float tau = 0.0f;
        if (!range_tau(metric, ld_, max_row_norm_, sq.norm, min_score, &tau)) tau = std::nanf("");
        const bool qarg = scan_range_takes_qarg(ld_);
        const float* q32 = qarg ? stage_q32(ws, query, dim_, ld_) : nullptr;
        const bool prof = profile_.load();
        ScanPlan plan;
        VL_HIP(hipMemsetAsync(ws->rg_ctr, 0, RANGE_CTR_WORDS * sizeof(uint32_t), st));
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        VL_HIP(launch_scan_range(st, metric, d_slab_, d_inv_norm_, plist, m, ws->d_q64, (uint32_t)dim_, ld_, tau, ws->rg_cand, cap,
                                 ws->rg_ctr, &plan, q32));
        if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
        VL_HIP(launch_range_rescore(st, metric, d_master_, ws->d_q64, ws->rg_cand, cap, (uint32_t)dim_, ws->rg_scores, ws->rg_ctr));
        VL_HIP(launch_range_cut(st, ws->rg_scores, ws->rg_cand, ws->rg_ctr + RANGE_CTR_APPENDED, cap, min_score, ws->rg_keys,
                                ws->rg_pv, cap, ws->rg_ctr));
        // up to RANGE_SMALL survivors are ranked and copied back before the host knows their number: one round trip
        const uint64_t k_spec = std::min<uint64_t>(out_capacity, RANGE_SMALL);
        VL_HIP(launch_range_rank(st, ws->rg_keys, ws->rg_pv, ws->rg_scores, ws->rg_ctr + RANGE_CTR_TOTAL, 0, k_spec, ws->d_out_pos,
                                 ws->d_out_scores));
        VL_HIP(hipMemcpyAsync(ws->rg_h_ctr, ws->rg_ctr, RANGE_CTR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (k_spec) {
            VL_HIP(hipMemcpyAsync(ws->rg_h_pos, ws->d_out_pos, k_spec * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            VL_HIP(hipMemcpyAsync(ws->rg_h_scores, ws->d_out_scores, k_spec * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        VL_HIP(hipStreamSynchronize(st));
        note_scan(plan.variant, plan.grid, qarg);
        if (prof)
            VL_TRY(account_profile(ws, m * ((uint64_t)ld_ * sizeof(float) + (plist ? sizeof(uint32_t) : 0) +
                                            (metric == COSINE ? sizeof(float) : 0))));
        const uint64_t appended = ws->rg_h_ctr[RANGE_CTR_APPENDED], total = ws->rg_h_ctr[RANGE_CTR_TOTAL];
        // in-domain rows cannot score NaN; a raised flag sends the call to the exact route, which decides the status
        if (appended <= cap && ws->rg_h_ctr[RANGE_CTR_NAN] == 0) {
            if (appended > m || total > appended) {
                set_last_error("range scan counted more rows than it was given (kernel bug)");
                return ERR_DEVICE;
            }
            const uint64_t want = std::min<uint64_t>(total, out_capacity);
            set_last_path(PATH_FAST);
            if (total <= RANGE_SMALL) return answer(ws->rg_h_pos, ws->rg_h_scores, want, total);
            std::vector<uint32_t> pos(want);
            std::vector<double> scores(want);
            if (want) {
                VL_TRY(ensure_range_ws(ws, RANGE_CAND_MAX, want));
                VL_HIP(launch_range_rank(st, ws->rg_keys, ws->rg_pv, ws->rg_scores, nullptr, total, want, ws->d_out_pos,
                                         ws->d_out_scores));
                VL_HIP(hipMemcpyAsync(pos.data(), ws->d_out_pos, want * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                VL_HIP(hipMemcpyAsync(scores.data(), ws->d_out_scores, want * sizeof(double), hipMemcpyDeviceToHost, st));
                VL_HIP(hipStreamSynchronize(st));
            }
            return answer(pos.data(), scores.data(), want, total);
        }
        // more candidates than the buffer holds: every score, then the cut
    }

    // the exact route: the reference score of every row, the cut, the sort on (score desc, position asc)
    VL_TRY(ensure_range_ws(ws, 0, 0));
    VL_TRY(ensure_scores(ws, m));
    VL_HIP(hipMemsetAsync(ws->rg_ctr, 0, RANGE_CTR_WORDS * sizeof(uint32_t), st));
    if (plist)
        VL_HIP(launch_exact_scan_subset(st, metric, d_master_, ws->d_q64, plist, m, (uint32_t)dim_, ws->d_scores,
                                        ws->rg_ctr + RANGE_CTR_NAN));
    else
        VL_HIP(launch_exact_scan(st, metric, d_master_, ws->d_q64, m, (uint32_t)dim_, ws->d_scores, ws->rg_ctr + RANGE_CTR_NAN));
    VL_HIP(launch_range_cut(st, ws->d_scores, plist, nullptr, m, min_score, nullptr, nullptr, 0, ws->rg_ctr));  // count only
    VL_HIP(hipMemcpyAsync(ws->rg_h_ctr, ws->rg_ctr, RANGE_CTR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VL_HIP(hipStreamSynchronize(st));
    if (ws->rg_h_ctr[RANGE_CTR_NAN] && m >= 2) {  // a 1-element sort never calls the comparator (and NaN >= x is false)
        set_last_error("NaN similarity score: the reference panics in partial_cmp().unwrap()");
        return ERR_NAN_SCORE;
    }
    const uint64_t total = ws->rg_h_ctr[RANGE_CTR_TOTAL];
    if (total > m) {
        set_last_error("range cut counted more rows than it was given (kernel bug)");
        return ERR_DEVICE;
    }
    const uint64_t want = std::min<uint64_t>(total, out_capacity);
    std::vector<uint32_t> pos(want);
    std::vector<double> scores(want);
    if (want) {
        VL_TRY(ensure_range_ws(ws, sort_capacity_for(total), want));
        VL_HIP(hipMemsetAsync(ws->rg_ctr + RANGE_CTR_TOTAL, 0, sizeof(uint32_t), st));
        VL_HIP(launch_range_cut(st, ws->d_scores, plist, nullptr, m, min_score, ws->rg_keys, ws->rg_pv, total, ws->rg_ctr));
        VL_HIP(launch_range_rank(st, ws->rg_keys, ws->rg_pv, ws->d_scores, nullptr, total, want, ws->d_out_pos, ws->d_out_scores));
        VL_HIP(hipMemcpyAsync(pos.data(), ws->d_out_pos, want * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipMemcpyAsync(scores.data(), ws->d_out_scores, want * sizeof(double), hipMemcpyDeviceToHost, st));
        VL_HIP(hipStreamSynchronize(st));
    }
    set_last_path(PATH_EXACT_SORT);
    return answer(pos.data(), scores.data(), want, total);
}

// ---------------------------------------------------------------------------------------------
// Grouped search (NEW): the best row of each of the best k groups.
//
// Pass 1 (k_scan_group_best) leaves the best f32 key of every group in best[]; the 64 largest are decoded and the first k
// rescored in the reference's order.  L = the smallest of those k scores: k distinct groups each hold a row scoring >= L,
// so the k-th group of the answer scores >= L, every row of the answer scores >= L, and in the ranking every row scoring
// >= L stands in front of every row scoring less -- the first k distinct groups of the ranking are decided inside the rows
// with score >= L.  Pass 2 is a range search at min_score = L (threshold ties in), its ranked survivors are collapsed on
// the device.  Nothing is certified; the exact route (every score, the sort, the same collapse) is taken for k > 64, fewer
// than k non-empty groups, a NaN, a candidate overflow, or data / query outside the fast-path domain.
// ---------------------------------------------------------------------------------------------
GroupTable::~GroupTable()
{
    (void)hipSetDevice(rows.device);
    void* dev[] = {d_dense, d_keys, d_group_of_row, d_keep};
    for (void* p : dev)
        if (p) (void)hipFree(p);
}

int GpuFlatIndex::find_groups(uint64_t token, std::shared_ptr<GroupTable>* out) const
{
    return token_find(filters_mu_, groups_, token, UNKNOWN_GROUPS, out);
}

int GpuFlatIndex::groups_create(GroupPlan&& plan, uint64_t* out_token, uint64_t* out_rows)
{
    if (!out_token || plan.ids.size() != plan.dense.size()) return ERR_INVALID_ARG;
    *out_token = 0;
    auto t = std::make_shared<GroupTable>();
    t->rows.device = device_;
    t->rows.ids = std::move(plan.ids);
    t->keys = std::move(plan.keys);
    VL_HIP(hipSetDevice(device_));
    const size_t ni = t->rows.ids.size();
    if (ni) {
        VL_TRY(dev_alloc(&t->rows.d_ids, ni));
        VL_HIP(hipMemcpy(t->rows.d_ids, t->rows.ids.data(), ni * sizeof(uint64_t), hipMemcpyHostToDevice));
        VL_TRY(dev_alloc(&t->rows.d_counts, (size_t)FILTER_COUNTS_MAX + 1));
        VL_TRY(dev_alloc(&t->d_dense, ni));
        VL_HIP(hipMemcpy(t->d_dense, plan.dense.data(), ni * sizeof(uint32_t), hipMemcpyHostToDevice));
        VL_TRY(dev_alloc(&t->d_keys, t->keys.size()));
        VL_HIP(hipMemcpy(t->d_keys, t->keys.data(), t->keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    uint64_t rows = 0;
    {
        std::shared_lock<RwLock> lk(mu_);
        std::lock_guard<std::mutex> tg(t->rows.mu);
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(resolve_groups(lease.ws, t.get())));
        rows = t->rows.m;
    }
    const uint64_t token = g_next_filter_token.fetch_add(1);
    {
        std::lock_guard<std::mutex> g(filters_mu_);
        groups_[token] = std::move(t);
    }
    *out_token = token;
    if (out_rows) *out_rows = rows;
    return OK;
}

int GpuFlatIndex::groups_destroy(uint64_t groups)
{
    std::shared_ptr<GroupTable> t;  // a search still using it holds its own reference: freed when that one ends
    return token_take(filters_mu_, groups_, groups, UNKNOWN_GROUPS, &t);
}

int GpuFlatIndex::groups_rows(uint64_t groups, uint64_t* out_rows, uint64_t* out_distinct) const
{
    if (!out_rows) return ERR_INVALID_ARG;
    std::shared_ptr<GroupTable> t;
    VL_TRY(find_groups(groups, &t));
    std::shared_lock<RwLock> lk(mu_);
    std::lock_guard<std::mutex> tg(t->rows.mu);
    if (t->rows.resolved_at != mutations_) {
        WsLease lease(this);
        if (lease.status() != OK) return lease.status();
        VL_TRY(lease.done(resolve_groups(lease.ws, t.get())));
    }
    *out_rows = t->rows.m;
    if (out_distinct) *out_distinct = t->keys.size();
    return OK;
}

// The filter's resolution over the table's ids (the ascending positions of the rows that have a group), then
// group_of_row[p] for every position.
int GpuFlatIndex::resolve_groups(Workspace* ws, GroupTable* t) const
{
    const uint64_t n = ids_.size();
    VL_TRY(resolve_filter(ws, &t->rows));
    t->rows.resolved_at = ~0ull;
    if (n != 0 && !t->rows.ids.empty()) {
        VL_TRY(grow(HipMem{}, t->gor_cap, n, {dev_buf(t->d_group_of_row, n)}));
        VL_HIP(launch_group_rows(ws->stream, d_ids_, n, t->rows.d_ids, t->d_dense, t->rows.ids.size(), t->d_group_of_row));
        VL_HIP(hipStreamSynchronize(ws->stream));
    }
    t->rows.resolved_at = mutations_;
    return OK;
}

int GpuFlatIndex::search_grouped(uint64_t groups, uint64_t token, const double* query, uint64_t q_len, uint64_t k, int metric,
                                 uint64_t out_capacity, uint64_t* out_group_keys, uint64_t* out_pos, uint64_t* out_ids,
                                 double* out_scores, uint64_t* out_n) const
{
    if (!out_n) return ERR_INVALID_ARG;
    *out_n = 0;
    set_last_path(PATH_NONE);  // an answer that needs no scan (k = 0, an empty index, an empty S) took no route
    if (k > GROUPED_MAX_K) {
        set_last_error("grouped search: k exceeds VL_GROUPED_MAX_K (1024)");
        return ERR_INVALID_ARG;
    }
    std::shared_ptr<GroupTable> t;
    VL_TRY(find_groups(groups, &t));
    std::shared_ptr<IdFilter> f;
    if (token != 0) VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk;
    VL_TRY(lock_for_query(metric, q_len, &lk));
    if (ids_.empty() || k == 0) return OK;
    if ((!query && dim_) || (out_capacity != 0 && (!out_scores || !out_group_keys))) return ERR_INVALID_ARG;
    return run_search(t.get(), f.get(), [&](Workspace* ws) -> int {
        if (t->rows.m == 0 || (f && f->m == 0)) return OK;
        return search_grouped_locked(ws, t.get(), f.get(), query, k, metric, out_capacity, out_group_keys, out_pos, out_ids, out_scores,
                                     out_n);
    });
}

int GpuFlatIndex::search_grouped_locked(Workspace* ws, const GroupTable* t, const IdFilter* f, const double* query, uint64_t k,
                                        int metric, uint64_t out_capacity, uint64_t* out_group_keys, uint64_t* out_pos,
                                        uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    const uint64_t n = ids_.size();
    // the rows scanned: the filter's list (rows without a group are dropped at the sinks and at the cut), else the table's
    // own list of grouped rows -- or every row when all of them have a group
    const uint32_t* plist = f ? f->d_plist : (t->rows.m == n ? nullptr : t->rows.d_plist);
    const uint64_t m = f ? f->m : t->rows.m;
    const uint32_t* gor = t->d_group_of_row;
    const uint64_t ng = t->keys.size();
    const uint32_t k32 = (uint32_t)k;
    hipStream_t st = ws->stream;

    const StagedQuery sq = stage_single_query(ws, query, dim_);
    VL_HIP(hipMemcpyAsync(ws->d_q64, ws->h_q64, (dim_ + 1) * sizeof(double), hipMemcpyHostToDevice, st));

    VL_TRY(ensure_group_ws(ws, ng));
    VL_TRY(ensure_range_ws(ws, 0, GROUPED_MAX_K));

    // the collapse of `total` ranked survivors (total_ptr: the count is still the device's) and its copy back
    auto collapse = [&](const double* scores, const uint32_t* total_ptr, uint64_t total) -> int {
        VL_HIP(launch_group_collapse(st, ws->rg_pv, scores, total_ptr, total, gor, n, reinterpret_cast<const uint64_t*>(t->d_keys), ng,
                                     ws->gp_first, k32, ws->gp_out_keys, ws->d_out_pos, ws->d_out_scores,
                                     ws->gp_ctr + RANGE_CTR_WORDS));
        VL_HIP(hipMemcpyAsync(ws->gp_h_ctr + RANGE_CTR_WORDS, ws->gp_ctr + RANGE_CTR_WORDS, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipMemcpyAsync(ws->gp_h_keys, ws->gp_out_keys, k * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipMemcpyAsync(ws->rg_h_pos, ws->d_out_pos, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipMemcpyAsync(ws->rg_h_scores, ws->d_out_scores, k * sizeof(double), hipMemcpyDeviceToHost, st));
        return OK;
    };
    // writes the answer from the pinned copies of the collapse's output
    auto answer = [&](uint64_t emitted) -> int {
        const uint64_t want = std::min<uint64_t>(emitted, out_capacity);
        VL_TRY(deliver("grouped search", ids_, ws->rg_h_pos, ws->rg_h_scores, want, out_pos, out_ids, out_scores));
        for (uint64_t i = 0; i < want; ++i) out_group_keys[i] = ws->gp_h_keys[i];
        *out_n = want;
        return OK;
    };

    const uint32_t cap = range_candidate_capacity();
    const bool fast_ok = force_path_.load() == 0 && n_out_of_domain_ == 0 && sq.in_domain && k <= (uint64_t)KP;
    while (fast_ok) {  // (one round: `break` leaves for the exact route)
        VL_TRY(ensure_range_ws(ws, RANGE_CAND_MAX, GROUPED_MAX_K));
        VL_TRY(ensure_range_candidates(ws));
        const bool qarg = scan_range_takes_qarg(ld_);
        const float* q32 = qarg ? stage_q32(ws, query, dim_, ld_) : nullptr;
        // pass 1: the best key of every group, the 64 best groups, the reference scores of the first k of them
        const bool prof = profile_.load();
        ScanPlan plan;
        VL_HIP(hipMemsetAsync(ws->gp_best, 0, ng * sizeof(uint64_t), st));
        VL_HIP(hipMemsetAsync(ws->gp_ctr, 0, (RANGE_CTR_WORDS + 1) * sizeof(uint32_t), st));
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        VL_HIP(launch_scan_group_best(st, metric, d_slab_, d_inv_norm_, plist, m, ws->d_q64, (uint32_t)dim_, ld_, gor, ws->gp_best,
                                      &plan, q32));
        if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
        VL_HIP(launch_group_top(st, ws->gp_best, ng, k32, ws->gp_lists, ws->gp_cand, ws->gp_ctr));
        VL_HIP(launch_range_rescore(st, metric, d_master_, ws->d_q64, ws->gp_cand, (uint32_t)KP, (uint32_t)dim_, ws->gp_scores,
                                    ws->gp_ctr));
        VL_HIP(hipMemcpyAsync(ws->gp_h_ctr, ws->gp_ctr, RANGE_CTR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipMemcpyAsync(ws->gp_h_scores, ws->gp_scores, k * sizeof(double), hipMemcpyDeviceToHost, st));
        VL_HIP(hipStreamSynchronize(st));
        note_scan(plan.variant, plan.grid, qarg);
        if (prof)
            VL_TRY(account_profile(ws, m * ((uint64_t)ld_ * sizeof(float) + sizeof(uint32_t) + (plist ? sizeof(uint32_t) : 0) +
                                            (metric == COSINE ? sizeof(float) : 0))));
        if (ws->gp_h_ctr[RANGE_CTR_APPENDED] < k || ws->gp_h_ctr[RANGE_CTR_NAN] != 0) break;  // fewer than k non-empty groups; a NaN
        double L = ws->gp_h_scores[0];
        bool nan = false;
        for (uint64_t i = 0; i < k; ++i) {
            const double sc = ws->gp_h_scores[i];
            if (sc != sc) nan = true;
            if (sc < L) L = sc;
        }
        if (nan) break;

        // pass 2: the range search at min_score = L, rows without a group dropped at the cut, and the collapse
        float tau = 0.0f;
        if (!range_tau(metric, ld_, max_row_norm_, sq.norm, L, &tau)) tau = std::nanf("");
        VL_HIP(hipMemsetAsync(ws->rg_ctr, 0, RANGE_CTR_WORDS * sizeof(uint32_t), st));
        VL_HIP(launch_scan_range(st, metric, d_slab_, d_inv_norm_, plist, m, ws->d_q64, (uint32_t)dim_, ld_, tau, ws->rg_cand, cap,
                                 ws->rg_ctr, nullptr, q32));
        VL_HIP(launch_range_rescore(st, metric, d_master_, ws->d_q64, ws->rg_cand, cap, (uint32_t)dim_, ws->rg_scores, ws->rg_ctr));
        VL_HIP(launch_range_cut(st, ws->rg_scores, ws->rg_cand, ws->rg_ctr + RANGE_CTR_APPENDED, cap, L, ws->rg_keys, ws->rg_pv, cap,
                                ws->rg_ctr, gor, n, false));
        // up to RANGE_SMALL survivors are ranked and collapsed before the host knows their number: one round trip
        VL_HIP(launch_range_rank(st, ws->rg_keys, ws->rg_pv, ws->rg_scores, ws->rg_ctr + RANGE_CTR_TOTAL, 0, 0, nullptr, nullptr));
        VL_TRY(collapse(ws->rg_scores, ws->rg_ctr + RANGE_CTR_TOTAL, RANGE_SMALL));
        VL_HIP(hipMemcpyAsync(ws->rg_h_ctr, ws->rg_ctr, RANGE_CTR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipStreamSynchronize(st));
        const uint64_t appended = ws->rg_h_ctr[RANGE_CTR_APPENDED], total = ws->rg_h_ctr[RANGE_CTR_TOTAL];
        if (appended > cap || ws->rg_h_ctr[RANGE_CTR_NAN] != 0) break;  // more candidates than the buffer holds; a NaN
        if (appended > m || total > appended) {
            set_last_error("range scan counted more rows than it was given (kernel bug)");
            return ERR_DEVICE;
        }
        if (total > RANGE_SMALL) {
            VL_HIP(launch_range_rank(st, ws->rg_keys, ws->rg_pv, ws->rg_scores, nullptr, total, 0, nullptr, nullptr));
            VL_TRY(collapse(ws->rg_scores, nullptr, total));
            VL_HIP(hipStreamSynchronize(st));
        }
        // the k rows behind L are among the survivors, so k groups are; should that ever fail, the exact route answers and
        // vl_last_path shows it
        if (ws->gp_h_ctr[RANGE_CTR_WORDS] != k) break;
        set_last_path(PATH_FAST);
        return answer(k);
    }

    // the exact route: the reference score of every row, the grouped rows ranked by the device-wide sort, the collapse
    VL_TRY(ensure_scores(ws, m));
    const double neg_inf = -std::numeric_limits<double>::infinity();
    VL_HIP(hipMemsetAsync(ws->rg_ctr, 0, RANGE_CTR_WORDS * sizeof(uint32_t), st));
    if (plist)
        VL_HIP(launch_exact_scan_subset(st, metric, d_master_, ws->d_q64, plist, m, (uint32_t)dim_, ws->d_scores,
                                        ws->rg_ctr + RANGE_CTR_NAN));
    else
        VL_HIP(launch_exact_scan(st, metric, d_master_, ws->d_q64, m, (uint32_t)dim_, ws->d_scores, ws->rg_ctr + RANGE_CTR_NAN));
    // count only: TOTAL = |S| (NaN scores of grouped rows stay in), GROUP_NAN = how many of them are NaN.  The scan's own
    // flag also covers filtered rows without a group, which are not rows of S.
    VL_HIP(launch_range_cut(st, ws->d_scores, plist, nullptr, m, neg_inf, nullptr, nullptr, 0, ws->rg_ctr, gor, n, true));
    VL_HIP(hipMemcpyAsync(ws->rg_h_ctr, ws->rg_ctr, RANGE_CTR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VL_HIP(hipStreamSynchronize(st));
    const uint64_t total = ws->rg_h_ctr[RANGE_CTR_TOTAL];
    if (total > m) {
        set_last_error("grouped cut counted more rows than it was given (kernel bug)");
        return ERR_DEVICE;
    }
    if (ws->rg_h_ctr[RANGE_CTR_GROUP_NAN] && total >= 2) {  // a 1-element sort never calls the comparator
        set_last_error("NaN similarity score: the reference panics in partial_cmp().unwrap()");
        return ERR_NAN_SCORE;
    }
    set_last_path(PATH_EXACT_SORT);
    if (total == 0) return OK;
    VL_TRY(ensure_range_ws(ws, sort_capacity_for(total), GROUPED_MAX_K));
    VL_HIP(hipMemsetAsync(ws->rg_ctr, 0, RANGE_CTR_WORDS * sizeof(uint32_t), st));
    VL_HIP(launch_range_cut(st, ws->d_scores, plist, nullptr, m, neg_inf, ws->rg_keys, ws->rg_pv, total, ws->rg_ctr, gor, n, true));
    VL_HIP(launch_range_rank(st, ws->rg_keys, ws->rg_pv, ws->d_scores, nullptr, total, 0, nullptr, nullptr));
    VL_TRY(collapse(ws->d_scores, nullptr, total));
    VL_HIP(hipStreamSynchronize(st));
    const uint64_t emitted = ws->gp_h_ctr[RANGE_CTR_WORDS];
    if (emitted > k) {
        set_last_error("grouped collapse emitted more rows than asked for (kernel bug)");
        return ERR_DEVICE;
    }
    return answer(emitted);
}

// ---------------------------------------------------------------------------------------------
// Batched grouped search: nq grouped queries against one index state.  The MFMA batch filter already
// leaves, per query, the 64 best rows of S rescored in the reference's order; k_batch_rank_collapse certifies as long a
// prefix of that ranking as the bound allows and collapses it to one row per group.  A query whose prefix holds k groups
// (or whose S fits the list) is settled without any per-group atomic; every other query runs the single search's body
// under the same lock, so each row is the single call's answer bit for bit.
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::grouped_keep_bits(Workspace* ws, GroupTable* t, IdFilter* f, const unsigned long long** keep, uint64_t* m) const
{
    const uint64_t n = ids_.size(), words = (n + 63) / 64;
    hipStream_t st = ws->stream;
    VL_TRY(ensure_set(HipMem{}, {dev_buf(ws->gb_m, 1)}));
    uint32_t m32 = 0;
    auto count = [&]() -> int {
        VL_HIP(hipMemcpyAsync(&m32, ws->gb_m, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipStreamSynchronize(st));
        return OK;
    };
    if (!f) {  // the table alone: cached on the table until rows are added or deleted
        std::lock_guard<std::mutex> g(t->rows.mu);
        if (t->keep_at != mutations_) {
            t->keep_at = ~0ull;
            VL_TRY(grow(HipMem{}, t->keep_cap, words, {dev_buf(t->d_keep, words)}));
            VL_HIP(launch_group_keep_bits(st, t->d_group_of_row, n, nullptr, nullptr, nullptr, 0, t->d_keep, ws->gb_m));
            VL_TRY(count());
            if (m32 != t->rows.m) {
                set_last_error("the group table's keep bitmap and its row list disagree (kernel bug)");
                return ERR_DEVICE;
            }
            t->keep_at = mutations_;
        }
        *keep = t->d_keep;
        *m = t->rows.m;
        return OK;
    }
    VL_TRY(grow(HipMem{}, ws->gb_keep_cap, words, {dev_buf(ws->gb_keep, words)}));
    if (f->has_keep()) {
        VL_HIP(launch_group_keep_bits(st, t->d_group_of_row, n, f->d_keep, nullptr, nullptr, 0, ws->gb_keep, ws->gb_m));
    } else {
        VL_TRY(ensure_device_ids());
        VL_HIP(launch_group_keep_bits(st, t->d_group_of_row, n, nullptr, d_ids_, f->d_ids, f->ids.size(), ws->gb_keep, ws->gb_m));
    }
    VL_TRY(count());
    if (m32 > t->rows.m || m32 > f->m) {
        set_last_error("the keep bitmap of a grouped batch holds more rows than its table or its filter (kernel bug)");
        return ERR_DEVICE;
    }
    *keep = ws->gb_keep;
    *m = m32;
    return OK;
}

int GpuFlatIndex::search_grouped_batch(uint64_t groups, uint64_t token, const double* queries, uint64_t nq, uint64_t q_len,
                                       uint64_t k, int metric, uint64_t out_stride, uint64_t* out_group_keys, uint64_t* out_ids,
                                       double* out_scores, uint64_t* out_n) const
{
    uint64_t gb[4] = {0, 0, 0, 0};  // last_grouped_batch: routed, settled, handed back, sequences
    auto publish = [&]() {
        for (int i = 0; i < 4; ++i) last_gbatch_[i].store(gb[i], std::memory_order_relaxed);
    };
    if (nq == 0) {
        publish();
        return OK;
    }
    if (!out_n) return ERR_INVALID_ARG;
    for (uint64_t i = 0; i < nq; ++i) out_n[i] = 0;
    set_last_path(PATH_NONE);
    if (k > GROUPED_MAX_K) {
        set_last_error("grouped search: k exceeds VL_GROUPED_MAX_K (1024)");
        return ERR_INVALID_ARG;
    }
    std::shared_ptr<GroupTable> t;
    VL_TRY(find_groups(groups, &t));
    std::shared_ptr<IdFilter> f;
    if (token != 0) VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk;  // one index state for the whole batch
    VL_TRY(lock_for_query(metric, q_len, &lk));
    if (k > out_stride) {
        set_last_error("grouped batch: k exceeds out_stride");
        return ERR_INVALID_ARG;
    }
    publish();
    if (ids_.empty() || k == 0) return OK;
    if ((!queries && dim_) || !out_scores || !out_group_keys || !out_ids) return ERR_INVALID_ARG;

    WsLease lease(this, /*sync_always=*/true);
    if (lease.status() != OK) return lease.status();
    Workspace* const ws = lease.ws;
    VL_TRY(resolve_if_stale(ws, t.get()));
    // an exclusion token's position list waits until a query is left to the single search: the pass reads a bitmap
    if (f) VL_TRY(resolve_if_stale(ws, f.get(), /*need_list=*/false));
    InFlight searching(active_searches_);
    if (t->rows.m == 0 || (f && f->m == 0)) return OK;  // an empty S (search_grouped's early return)

    const uint64_t n = ids_.size();
    std::vector<uint8_t> done(nq, 0);
    {
        const char* mf_env = getenv("VL_MFMA");
        const char* mf_min = getenv("VL_MFMA_MIN_BATCH");
        const MaskedBatchLimits lim{MFMA_MIN_ROWS, mf_min && *mf_min ? (uint64_t)atoi(mf_min) : (uint64_t)MFMA_MIN_BATCH,
                                    (uint64_t)KFAST_MAX, mfma_sequence_queries((uint32_t)dim_)};
        GroupedBatchShape shp;
        shp.index = {force_path_.load() == 0 && n_out_of_domain_ == 0 && dim_ != 0 && !(mf_env && mf_env[0] == '0') &&
                         mfma_scan_supported((uint32_t)dim_, metric),
                     n, (uint32_t)dim_, ld_, mfma_ldb((uint32_t)dim_)};
        shp.rows_kernel = mfma_rows_kernel((uint32_t)dim_);
        shp.needs_bitmap = f != nullptr || t->rows.m != n;
        shp.m = f ? std::min<uint64_t>(t->rows.m, f->m) : t->rows.m;  // an upper bound until the bitmap is counted
        const int mode = grouped_batch_.load();
        // (the loop's estimate grows with m: a batch that loops at the upper bound loops at the counted m as well)
        if (grouped_batch_route(mode, shp, lim, nq, k)) {
            const unsigned long long* keep = nullptr;
            if (shp.needs_bitmap) {
                VL_TRY(grouped_keep_bits(ws, t.get(), f.get(), &keep, &shp.m));
                if (shp.m == 0) return OK;  // the filter keeps no grouped row
            }
            if (grouped_batch_route(mode, shp, lim, nq, k)) {
                std::vector<uint32_t> qidx, mq, kq;
                std::vector<const unsigned long long*> keep_of;
                MaskedQueries desc{nullptr, nullptr, nullptr, nullptr};
                if (keep) {  // every query of every sequence under the ONE bitmap of S
                    qidx.resize(nq);
                    for (uint64_t i = 0; i < nq; ++i) qidx[i] = (uint32_t)i;
                    mq.assign(nq, (uint32_t)shp.m);
                    kq.assign(nq, (uint32_t)k);
                    keep_of.assign(nq, keep);
                    desc = {qidx.data(), keep_of.data(), mq.data(), kq.data()};
                }
                const GroupedReq req{t.get(), shp.m, out_stride, out_group_keys};
                VL_TRY(search_batch_mfma(ws, queries, nullptr, nq, out_stride, k, metric, nullptr, out_ids, out_scores, out_n, &done,
                                         nullptr, keep ? &desc : nullptr, &gb[3], &req));
                gb[0] = nq;
                for (uint64_t qi = 0; qi < nq; ++qi) gb[1] += done[qi] ? 1 : 0;
                gb[2] = gb[0] - gb[1];
            }
        }
    }
    // what the pass did not settle (or everything), in ascending order: the first failure is the lowest failing query
    bool list_ready = !(f && f->lazy_list());
    for (uint64_t qi = 0; qi < nq; ++qi) {
        if (done[qi]) continue;
        if (!list_ready) {
            std::lock_guard<std::mutex> fg(f->mu);
            VL_TRY(ensure_plist(ws, f.get()));
            list_ready = true;
        }
        VL_TRY(search_grouped_locked(ws, t.get(), f.get(), queries + qi * dim_, k, metric, out_stride, out_group_keys + qi * out_stride,
                                     nullptr, out_ids + qi * out_stride, out_scores + qi * out_stride, out_n + qi));
    }
    if (gb[1]) set_last_path(PATH_FAST);
    publish();
    return OK;
}

// ---------------------------------------------------------------------------------------------
// large batches: bf16 MFMA candidate filter (mfma_scan.hip) + the same exact finalize
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::ensure_bf16_slab(bool frag_major) const
{
    std::lock_guard<std::mutex> g(bf16_mu_);
    const uint64_t n = ids_.size();
    const uint32_t ldb = mfma_ldb((uint32_t)dim_);
    // whole MFMA tiles: the batch kernels read the last, partial tile past the live rows (and mask them)
    const size_t cap16 = (cap_ + MFMA_TILE_ROWS - 1) / MFMA_TILE_ROWS * MFMA_TILE_ROWS;
    auto fail = [&](hipError_t e) {
        (void)hipGetLastError();
        set_last_error(std::string("bf16 slab allocation failed: ") + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? (int)ERR_OOM : (int)ERR_DEVICE;
    };
    if (!d_norm16_) {  // both per-row arrays or neither: a half-made set would be launched with null pointers next time
        float* sq = nullptr;
        float* nr = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&sq), cap16 * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&nr), cap16 * sizeof(float));
        if (e != hipSuccess) {
            if (sq) (void)hipFree(sq);
            if (nr) (void)hipFree(nr);
            return fail(e);
        }
        d_sqnorm_ = sq;
        d_norm16_ = nr;
    }
    void*& slab = frag_major ? d_slab16f_ : d_slab16_;
    uint64_t& rows_done = frag_major ? slab16f_rows_ : slab16_rows_;
    if (!slab) {
        void* s16 = nullptr;
        const hipError_t e = hipMalloc(&s16, cap16 * (size_t)ldb * 2);
        if (e != hipSuccess) return fail(e);
        slab = s16;
        rows_done = 0;
    }
    if (rows_done < n) {
        if (frag_major) {
            // the fragment layout interleaves 16 neighbouring rows: conversion restarts at the group boundary
            const uint64_t first = rows_done & ~15ull;
            VL_HIP(launch_rows_bf16_frag(mut_stream_, d_master_ + first * dim_, first, n - first, (uint32_t)dim_, slab, d_norm16_,
                                         d_sqnorm_));
        } else {
            char* dst = reinterpret_cast<char*>(slab) + rows_done * (size_t)ldb * 2;
            VL_HIP(launch_rows_bf16(mut_stream_, d_master_ + rows_done * dim_, n - rows_done, (uint32_t)dim_, dst,
                                    d_norm16_ + rows_done, d_sqnorm_ + rows_done));
        }
        VL_HIP(hipStreamSynchronize(mut_stream_));
        rows_done = n;
    }
    return OK;
}

// The int8 copy of the single-query filter: allocated all at once (the three arrays or none), converted from the f64
// master incrementally (rows added since the last build; a delete rewinds slab8_rows_, growth frees the copy).
int GpuFlatIndex::ensure_i8_slab() const
{
    std::lock_guard<std::mutex> g(bf16_mu_);
    const uint64_t n = ids_.size();
    const uint32_t ldb = mfma_ldb((uint32_t)dim_);
    if (!d_slab8_) {
        void* s8 = nullptr;
        float* sr = nullptr;
        float* nr = nullptr;
        hipError_t e = hipMalloc(&s8, cap_ * (size_t)ldb);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&sr), cap_ * 2 * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&nr), cap_ * sizeof(float));
        if (e != hipSuccess) {
            if (s8) (void)hipFree(s8);
            if (sr) (void)hipFree(sr);
            if (nr) (void)hipFree(nr);
            (void)hipGetLastError();
            set_last_error(std::string("int8 slab allocation failed: ") + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? (int)ERR_OOM : (int)ERR_DEVICE;
        }
        d_slab8_ = s8;
        d_sr8_ = sr;
        d_norm8_ = nr;
        slab8_rows_ = 0;
    }
    if (slab8_rows_ < n) {
        char* dst = reinterpret_cast<char*>(d_slab8_) + slab8_rows_ * (size_t)ldb;
        VL_HIP(launch_rows_i8(mut_stream_, d_master_ + slab8_rows_ * dim_, n - slab8_rows_, (uint32_t)dim_, dst,
                              d_sr8_ + 2 * slab8_rows_, d_norm8_ + slab8_rows_));
        VL_HIP(hipStreamSynchronize(mut_stream_));
        slab8_rows_ = n;
    }
    return OK;
}

// position -> id on the device, for exchange records written by the finalize kernel (search_batch_to_record).  Caller holds
// mu_ (shared or unique); concurrent callers serialise on bf16_mu_ like the other lazily built device copies.
int GpuFlatIndex::ensure_device_ids() const
{
    std::lock_guard<std::mutex> g(bf16_mu_);
    const uint64_t n = ids_.size();
    if (d_ids_cap_ < n) {
        unsigned long long* fresh = nullptr;
        const uint64_t want = std::max<uint64_t>(cap_, n);
        VL_HIP(hipMalloc(reinterpret_cast<void**>(&fresh), want * sizeof(unsigned long long)));
        if (d_ids_) (void)hipFree(d_ids_);
        d_ids_ = fresh;
        d_ids_cap_ = want;
        d_ids_rows_ = 0;
    }
    if (d_ids_rows_ < n) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64 ids");
        VL_HIP(hipMemcpyAsync(d_ids_ + d_ids_rows_, ids_.data() + d_ids_rows_, (n - d_ids_rows_) * sizeof(uint64_t),
                              hipMemcpyHostToDevice, mut_stream_));
        VL_HIP(hipStreamSynchronize(mut_stream_));
        d_ids_rows_ = n;
    }
    return OK;
}

int GpuFlatIndex::search_batch_to_record(const double* queries, bool queries_on_device, uint64_t nq, uint64_t q_len, uint64_t ks,
                                         int metric, uint64_t row_offset, unsigned long long* d_record, bool* handled) const
{
    if (handled) *handled = false;
    if (!handled || !d_record || nq == 0 || ks == 0 || !queries || metric < 0 || metric > 3) return OK;  // the host path decides
    VL_HIP(hipSetDevice(device_));
    std::shared_lock<RwLock> lk(mu_);
    const uint64_t n = ids_.size();
    if (n == 0 || q_len != dim_) return OK;  // (errors and empty shards are the host path's to report)
    const uint64_t k_eff = std::min<uint64_t>(ks, n);
    const char* mf_env = getenv("VL_MFMA");
    const char* mf_min = getenv("VL_MFMA_MIN_BATCH");
    const uint64_t mfma_min = mf_min && *mf_min ? (uint64_t)atoi(mf_min) : (uint64_t)MFMA_MIN_BATCH;
    const bool direct = nq > 1 && force_path_.load() == 0 && k_eff <= (uint64_t)KFAST_MAX && n_out_of_domain_ == 0 &&
                        !(mf_env && mf_env[0] == '0') && nq >= mfma_min && n >= MFMA_MIN_ROWS &&
                        mfma_scan_supported((uint32_t)dim_, metric) && nq * ks < (1ull << 31);
    if (!direct) return OK;
    VL_TRY(ensure_device_ids());
    ShardRecordSink sink;
    sink.cnt = d_record + SHARD_HDR_WORDS;
    sink.score_bits = sink.cnt + nq;
    sink.gpos = sink.score_bits + nq * ks;
    sink.ids = sink.gpos + nq * ks;
    sink.pos_to_id = d_ids_;
    sink.row_offset = row_offset;
    sink.ks = (uint32_t)ks;
    // host-side answers of the queries the filter certifies are not needed (the record is the answer); the others come back
    // through `done` and are redone below
    std::vector<uint8_t> done(nq, 0);
    std::vector<uint64_t> cnt(nq, 0);
    std::vector<uint64_t> pos, ids;
    std::vector<double> sc;
    try {
        pos.resize(nq * ks);
        ids.resize(nq * ks);
        sc.resize(nq * ks);
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory in the shard search");
        return ERR_OOM;
    }
    {
        WsLease lease(this, /*sync_always=*/true);
        if (lease.status() != OK) return lease.status();
        VL_TRY(search_batch_mfma(lease.ws, queries_on_device ? nullptr : queries, queries_on_device ? queries : nullptr, nq, ks, k_eff, metric,
                                 pos.data(), ids.data(), sc.data(), cnt.data(), &done, &sink));
    }
    set_last_path(PATH_FAST);
    // what the filter could not certify: the host paths answer those queries (under the same shared lock: one index state
    // for the whole batch) and their slices of the record are patched; typically none
    std::vector<uint64_t> left;
    for (uint64_t qi = 0; qi < nq; ++qi)
        if (!done[qi]) left.push_back(qi);
    if (!left.empty()) {
        const uint64_t m = left.size();
        std::vector<double> hq(m * dim_);
        for (uint64_t i = 0; i < m; ++i) {
            if (queries_on_device)
                VL_HIP(hipMemcpy(hq.data() + i * dim_, queries + left[i] * dim_, dim_ * sizeof(double), hipMemcpyDeviceToHost));
            else
                std::memcpy(hq.data() + i * dim_, queries + left[i] * dim_, dim_ * sizeof(double));
        }
        std::vector<uint64_t> t_pos(m * ks), t_ids(m * ks), t_n(m, 0);
        std::vector<double> t_sc(m * ks);
        VL_TRY(search_batch_locked(hq.data(), m, dim_, ks, metric, t_pos.data(), t_ids.data(), t_sc.data(), t_n.data()));
        for (uint64_t i = 0; i < m; ++i) {
            const uint64_t qi = left[i], c = std::min<uint64_t>(t_n[i], ks);
            std::vector<unsigned long long> buf(3 * ks, 0ull);
            for (uint64_t j = 0; j < c; ++j) {
                std::memcpy(&buf[j], &t_sc[i * ks + j], 8);
                buf[ks + j] = t_pos[i * ks + j] + row_offset;
                buf[2 * ks + j] = t_ids[i * ks + j];
            }
            const unsigned long long c64 = c;
            VL_HIP(hipMemcpy(sink.cnt + qi, &c64, 8, hipMemcpyHostToDevice));
            VL_HIP(hipMemcpy(sink.score_bits + qi * ks, buf.data(), ks * 8, hipMemcpyHostToDevice));
            VL_HIP(hipMemcpy(sink.gpos + qi * ks, buf.data() + ks, ks * 8, hipMemcpyHostToDevice));
            VL_HIP(hipMemcpy(sink.ids + qi * ks, buf.data() + 2 * ks, ks * 8, hipMemcpyHostToDevice));
        }
    }
    *handled = true;
    return OK;
}

int GpuFlatIndex::ensure_mfma_scratch(Workspace* ws) const
{
    if (ws->mf.nq_cap) return OK;
    const size_t nqc = MFMA_MAX_BATCH;
    const uint32_t ldb = mfma_ldb((uint32_t)dim_);
    const size_t nqp = nqc + 256;  // whole query chunks (128 / 96 / 256 queries) past the last query
    VL_HIP(hipMalloc(&ws->mf.q_bf16, nqp * ldb * 2));
    VL_TRY(dev_alloc(&ws->mf.gmax, nqc * MFMA_GROUPS));
    VL_TRY(dev_alloc(&ws->mf.thr, nqc));
    VL_TRY(dev_alloc(&ws->mf.cand, nqc * MFMA_CAND_CAP));
    VL_TRY(dev_alloc(&ws->mf.cnt, nqp));
    // per query: the f64 query, its norm, and (a masked batch) a bitmap pointer and the two words m, k
    VL_TRY(dev_alloc(&ws->mf_d_q64, nqc * (dim_ + 3)));
    VL_TRY(pinned_alloc(&ws->mf_h_q64, nqc * (dim_ + 3)));
    VL_TRY(dev_alloc(&ws->mf_lists, nqc * KP));
    VL_TRY(dev_alloc(&ws->mf_scores, nqc * KP));
    VL_TRY(pinned_alloc(&ws->mf_h_result, 2 * nqc));  // two launch sequences in flight: one being unpacked, one on the GPU
    VL_TRY(pinned_alloc(&ws->mf_h_dom, 2 * nqc));
    for (auto& e : ws->mf_ev_done) VL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    VL_HIP(hipEventCreateWithFlags(&ws->mf_ev_h2d, hipEventDisableTiming));
    ws->mf.nq_cap = (uint32_t)nqc;
    ws->mf.nq_pad_cap = (uint32_t)nqp;
    return OK;
}

// Cosine / dot / Euclidean batches of >= MFMA_MIN_BATCH queries.  done[qi] is set for every query
// answered here; the caller redoes the others (bound check failed, candidate overflow, ...).
int GpuFlatIndex::search_batch_mfma(Workspace* ws, const double* queries, const double* d_queries, uint64_t nq,
                                    uint64_t k, uint64_t k_eff, int metric, uint64_t* out_pos, uint64_t* out_ids,
                                    double* out_scores, uint64_t* out_n, std::vector<uint8_t>* done,
                                    const ShardRecordSink* sink, const MaskedQueries* masked, uint64_t* n_sequences,
                                    const GroupedReq* grouped, const MmrBatchReq* mmr) const
{
    static_assert(sizeof(const unsigned long long*) == sizeof(double) && 2 * sizeof(uint32_t) == sizeof(double),
                  "the masked descriptor is staged as two words per query behind the norms");
    if (masked && (d_queries || sink || !mfma_rows_kernel((uint32_t)dim_))) return ERR_INVALID_ARG;
    if (grouped && (d_queries || sink || !out_ids || !grouped->out_keys || k_eff == 0 || k_eff > (uint64_t)KFAST_MAX))
        return ERR_INVALID_ARG;
    if (mmr && (grouped || d_queries || sink || k_eff != mmr->n || mmr->n == 0 || mmr->n > (uint64_t)KFAST_MAX || mmr->n > mmr->m ||
                mmr->k_out == 0 || mmr->k_out > mmr->n || mmr->k_out > mmr->out_stride))
        return ERR_INVALID_ARG;
    if (n_sequences) *n_sequences = 0;
    const uint64_t n = ids_.size();
    const bool frag = mfma_rows_kernel((uint32_t)dim_);  // which kernel, hence which slab layout
    VL_TRY(ensure_bf16_slab(frag));
    const void* slab16 = frag ? d_slab16f_ : d_slab16_;
    VL_TRY(ensure_mfma_scratch(ws));
    if (grouped) VL_TRY(ensure_set(HipMem{}, {pinned_buf(ws->gb_h_result, 2 * (size_t)MFMA_MAX_BATCH)}));
    if (mmr) VL_TRY(ensure_set(HipMem{}, {dev_buf(ws->mb_ranked, (size_t)MFMA_MAX_BATCH)}));
    hipStream_t st = ws->stream;
    const double in_extra = IN_EXTRA_MFMA;  // bf16 rows and queries (mfma_scan.hpp)
    const uint64_t k_eff_all = k_eff;       // (a masked batch has its own per query)
    const bool prof = profile_.load();
    static const bool trace = getenv("VL_TRACE_BATCH") != nullptr;  // diagnostic: host-side phases of a sequence on stderr
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count();
    };
    const uint64_t seq = mfma_sequence_queries((uint32_t)dim_);
    // Launch sequences run as a two-deep pipeline: sequence s + 1 is staged and enqueued BEFORE the host waits for
    // sequence s, so the GPU goes from one sequence's finalize straight into the next one's filter while the host
    // unpacks result blocks (config 5 = two sequences of 2048 queries: rounds 1-3 ran them back to back with a stream
    // sync, the unpacking and the next staging in between).  Device buffers are shared: stream order keeps one sequence's
    // kernels behind the previous one's.  What the host touches comes in two copies (result blocks, in-domain flags), and
    // the one pinned staging area of host queries is reused only after its copies have left (ev_h2d).
    struct SeqState {
        uint64_t q0 = 0;
        uint32_t g = 0;
        bool live = false;
        std::vector<uint8_t> in_domain;
        std::chrono::steady_clock::time_point t0, t1, t2;
    } sq[2];
    const bool pipelined = !prof;  // (the profile's event pair brackets one sequence at a time)
    auto enqueue = [&](int slot, uint64_t q0) -> int {
        SeqState& S = sq[slot];
        S.q0 = q0;
        S.g = (uint32_t)std::min<uint64_t>(seq, nq - q0);
        S.live = true;
        S.t0 = now();
        const uint32_t g = S.g;
        S.in_domain.assign(g, 0);
        SearchResultBlock* res = ws->mf_h_result + (size_t)slot * MFMA_MAX_BATCH;
        unsigned char* dom = ws->mf_h_dom + (size_t)slot * MFMA_MAX_BATCH;
        bool prepared = false;
        if (d_queries) {  // already on this GPU: staged by a kernel; the flags land in pinned memory, read after the wait
            hipError_t pe = hipSuccess;
            prepared = frag && launch_prepare_queries(st, d_queries + q0 * dim_, g, (uint32_t)dim_, DOMAIN_MAX_ABS, DOMAIN_MIN_NORM,
                                                      ws->mf_d_q64, ws->mf_d_q64 + (size_t)g * dim_, dom, ws->mf, &pe);
            VL_HIP(pe);
            if (!prepared)
                VL_HIP(launch_stage_queries(st, d_queries + q0 * dim_, g, (uint32_t)dim_, DOMAIN_MAX_ABS, DOMAIN_MIN_NORM,
                                            ws->mf_d_q64, ws->mf_d_q64 + (size_t)g * dim_, dom));
        } else {
            // Host queries go to pinned memory (domain test, norm) and over PCIe in pieces: the copy of one piece runs
            // while the host stages the next, so a 6.3 MB batch (1024 x 768) costs about its staging time alone
            // (170 us) instead of staging + copy (170 + 115 us) in front of the first kernel.
            if (ws->mf_h2d_pending) {  // the previous sequence's copies out of this staging area
                VL_HIP(hipEventSynchronize(ws->mf_ev_h2d));
                ws->mf_h2d_pending = false;
            }
            double* norms = ws->mf_h_q64 + (size_t)g * dim_;
            const uint32_t piece = (uint32_t)std::max<uint64_t>(16, (1u << 20) / (dim_ * sizeof(double)));  // ~1 MB
            for (uint32_t j0 = 0; j0 < g; j0 += piece) {
                const uint32_t j1 = std::min<uint32_t>(g, j0 + piece);
                for (uint32_t j = j0; j < j1; ++j) {
                    const uint64_t src = masked ? masked->qidx[q0 + j] : q0 + j;
                    S.in_domain[j] = stage_query(queries + src * dim_, ws->mf_h_q64 + (size_t)j * dim_, dim_, &norms[j]) ? 1 : 0;
                }
                VL_HIP(hipMemcpyAsync(ws->mf_d_q64 + (size_t)j0 * dim_, ws->mf_h_q64 + (size_t)j0 * dim_,
                                      (size_t)(j1 - j0) * dim_ * sizeof(double), hipMemcpyHostToDevice, st));
            }
            // a masked batch: the sequence's bitmap table and its (m, k) words travel with the norms, in stream order with
            // the queries -- the two-deep pipeline shares the device copy like every other staging buffer
            if (masked) {
                const unsigned long long** h_keep = reinterpret_cast<const unsigned long long**>(norms + g);
                uint32_t* h_m = reinterpret_cast<uint32_t*>(norms + 2 * (size_t)g);
                for (uint32_t j = 0; j < g; ++j) {
                    h_keep[j] = masked->keep[q0 + j];
                    h_m[j] = masked->m[q0 + j];
                    h_m[g + j] = masked->k[q0 + j];
                }
            }
            VL_HIP(hipMemcpyAsync(ws->mf_d_q64 + (size_t)g * dim_, norms, (size_t)g * (masked ? 3 : 1) * sizeof(double),
                                  hipMemcpyHostToDevice, st));
            VL_HIP(hipEventRecord(ws->mf_ev_h2d, st));
            ws->mf_h2d_pending = true;
        }
        S.t1 = now();
        if (prof) VL_HIP(hipEventRecord(ws->ev0, st));
        MfmaLaunchInfo li;
        const double* d_norms = ws->mf_d_q64 + (size_t)g * dim_;
        const unsigned long long* const* d_keep_of = reinterpret_cast<const unsigned long long* const*>(d_norms + g);
        const uint32_t* d_m = reinterpret_cast<const uint32_t*>(d_norms + 2 * (size_t)g);
        if (masked)
            VL_HIP(launch_mfma_candidates_masked(st, metric, slab16, d_norm16_, d_sqnorm_, ws->mf_d_q64, g, n, (uint32_t)dim_,
                                                 ws->mf, d_keep_of, ws->mf_lists, &li));
        else
            VL_HIP(launch_mfma_candidates(st, metric, slab16, d_norm16_, d_sqnorm_, ws->mf_d_q64, g, n, (uint32_t)dim_,
                                          ws->mf, ws->mf_lists, &li, prepared));
        if (!masked) {
            const int v[6] = {li.ksteps, li.metric, li.chunks, li.grid_x, li.stages, li.sample_blocks};
            for (int i = 0; i < 6; ++i) last_filter_[i].store(v[i], std::memory_order_relaxed);
        }
        if (prof) VL_HIP(hipEventRecord(ws->ev1, st));
        ShardRecordSink seq_sink;
        if (sink) {  // this sequence's queries sit at [q0, q0 + g) of the record
            seq_sink = *sink;
            seq_sink.q0 = (uint32_t)q0;
        }
        // batches: the rescoring split over four workgroups per query + a rank / emit launch (launch_batch_finalize); a handful
        // of queries keeps the one-workgroup-per-query kernel (one launch less)
        static const bool split_off = []() { const char* v = getenv("VL_BATCH_FINALIZE"); return v && v[0] == '0'; }();
        if (grouped)  // the certified prefix of each list, collapsed to one row per group
            VL_HIP(launch_batch_finalize_grouped(st, metric, ws->mf_lists, (int)g, d_master_, ws->mf_d_q64, d_norms, (uint32_t)dim_,
                                                 grouped->m, (uint32_t)k_eff, max_row_norm_, grouped->table->d_group_of_row, n,
                                                 ws->gb_h_result + (size_t)slot * MFMA_MAX_BATCH, in_extra, ws->mf_scores));
        else if (mmr) {  // the certified prefix of each list, then similarities and selection
            VL_HIP(launch_batch_rescore(st, metric, ws->mf_lists, (int)g, d_master_, ws->mf_d_q64, (uint32_t)dim_, ws->mf_scores));
            VL_HIP(launch_mmr_batch(st, metric, ws->mf_lists, ws->mf_scores, (int)g, d_norms, d_master_, (uint32_t)dim_, mmr->m, n,
                                    (uint32_t)mmr->n, (uint32_t)mmr->k_out, mmr->lambda, max_row_norm_, in_extra, ws->mb_ranked, res));
        } else if (masked)  // the certificate per query: n_rows = m_q, k = min(k, m_q) (DESIGN.md sections 23, 24)
            VL_HIP(launch_batch_finalize_rows(st, metric, ws->mf_lists, (int)g, d_master_, ws->mf_d_q64, d_norms, (uint32_t)dim_,
                                              d_m, d_m + g, max_row_norm_, res, in_extra, ws->mf_scores));
        else if (g >= 8 && !split_off)
            VL_HIP(launch_batch_finalize(st, metric, ws->mf_lists, (int)g, d_master_, ws->mf_d_q64, ws->mf_d_q64 + (size_t)g * dim_,
                                         (uint32_t)dim_, n, (uint32_t)k_eff, max_row_norm_, res, in_extra, ws->mf_scores,
                                         sink ? &seq_sink : nullptr));
        else
            VL_HIP(launch_merge_finalize(st, metric, ws->mf_lists, 1, (int)g, d_master_, ws->mf_d_q64,
                                         ws->mf_d_q64 + (size_t)g * dim_, (uint32_t)dim_, n, (uint32_t)k_eff, max_row_norm_,
                                         res, in_extra, 0, sink ? &seq_sink : nullptr));
        VL_HIP(hipEventRecord(ws->mf_ev_done[slot], st));
        if (n_sequences) ++*n_sequences;
        S.t2 = now();
        return OK;
    };
    auto consume = [&](int slot) -> int {
        SeqState& S = sq[slot];
        if (!S.live) return OK;
        S.live = false;
        const uint32_t g = S.g;
        const SearchResultBlock* res = ws->mf_h_result + (size_t)slot * MFMA_MAX_BATCH;
        const unsigned char* dom = ws->mf_h_dom + (size_t)slot * MFMA_MAX_BATCH;
        VL_HIP(hipEventSynchronize(ws->mf_ev_done[slot]));
        if (d_queries)
            for (uint32_t j = 0; j < g; ++j) S.in_domain[j] = dom[j];
        const auto t_3 = now();
        if (prof) {
            uint64_t bytes = n * (uint64_t)mfma_ldb((uint32_t)dim_) * 2;
            if (masked) {  // and every distinct bitmap of the sequence once
                std::vector<const unsigned long long*> maps(masked->keep + S.q0, masked->keep + S.q0 + g);
                std::sort(maps.begin(), maps.end());
                bytes += (uint64_t)(std::unique(maps.begin(), maps.end()) - maps.begin()) * (n / 8);
            }
            VL_TRY(account_profile(ws, bytes));
        }
        for (uint32_t j = 0; grouped && j < g; ++j) {  // settled queries: position -> id, group number -> key
            const uint64_t qi = S.q0 + j;
            const GroupedResultBlock& r = ws->gb_h_result[(size_t)slot * MFMA_MAX_BATCH + j];
            if (!S.in_domain[j] || r.flags != 0u) continue;
            const std::vector<uint64_t>& keys = grouped->table->keys;
            bool ok = r.n_out <= k_eff_all;
            for (uint64_t i = 0; ok && i < r.n_out; ++i) ok = r.pos[i] < n && r.group[i] < keys.size();
            if (!ok) {
                set_last_error("grouped MFMA path returned an out-of-range entry (kernel bug)");
                return ERR_DEVICE;
            }
            const uint64_t want = std::min<uint64_t>(r.n_out, grouped->out_stride);
            for (uint64_t i = 0; i < want; ++i) {
                const size_t o = qi * grouped->out_stride + i;
                grouped->out_keys[o] = keys[r.group[i]];
                if (out_pos) out_pos[o] = r.pos[i];
                out_ids[o] = ids_[r.pos[i]];
                out_scores[o] = r.score[i];
            }
            out_n[qi] = want;
            (*done)[qi] = 1;
        }
        for (uint32_t j = 0; mmr && j < g; ++j) {  // settled queries: the selection, position -> id
            const uint64_t qi = S.q0 + j;
            const SearchResultBlock& r = res[j];
            if (!S.in_domain[j] || r.flags != 0u) continue;
            bool ok = r.n_out == mmr->k_out;
            for (uint64_t i = 0; ok && i < mmr->k_out; ++i) ok = r.pos[i] < n;
            if (!ok) {
                set_last_error("the batched selection returned an out-of-range entry (kernel bug)");
                return ERR_DEVICE;
            }
            for (uint64_t i = 0; i < mmr->k_out; ++i) {
                const size_t o = qi * mmr->out_stride + i;
                if (out_pos) out_pos[o] = r.pos[i];
                if (out_ids) out_ids[o] = ids_[r.pos[i]];
                out_scores[o] = r.score[i];
            }
            out_n[qi] = mmr->k_out;
            (*done)[qi] = 1;
        }
        for (uint32_t j = 0; !grouped && !mmr && j < g; ++j) {
            const uint64_t qi = S.q0 + j;
            const SearchResultBlock& r = res[j];
            const uint64_t k_eff = masked ? masked->k[qi] : k_eff_all;
            if (!S.in_domain[j] || (r.flags & RESULT_NEEDS_EXACT) || r.n_out != k_eff) continue;
            bool ok = true;
            for (uint64_t i = 0; i < k_eff; ++i) ok = ok && r.pos[i] < n;
            if (!ok) {
                set_last_error("MFMA path returned an out-of-range position (kernel bug)");
                return ERR_DEVICE;
            }
            for (uint64_t i = 0; i < k_eff; ++i) {
                const uint32_t p = r.pos[i];
                if (out_pos) out_pos[qi * k + i] = p;
                if (out_ids) out_ids[qi * k + i] = ids_[p];
                out_scores[qi * k + i] = r.score[i];
            }
            out_n[qi] = k_eff;
            (*done)[qi] = 1;
        }
        if (trace) {
            const auto t4 = now();
            fprintf(stderr, "[vl batch] %u queries: stage %ld us, enqueue %ld us, wait %ld us, unpack %ld us\n", g, us(S.t0, S.t1),
                    us(S.t1, S.t2), us(S.t2, t_3), us(t_3, t4));
        }
        return OK;
    };
    int rc = OK;
    int slot = 0;
    for (uint64_t q0 = 0; q0 < nq && rc == OK; q0 += seq, slot ^= 1) {
        rc = consume(slot);  // the sequence that used this slot's host buffers two steps ago (nothing on the first two turns)
        if (rc == OK) rc = enqueue(slot, q0);
        if (rc == OK && !pipelined) rc = consume(slot);
    }
    // drain (also on an error: nothing of this call may still be writing result blocks when the workspace goes back)
    for (int d = 0; d < 2; ++d, slot ^= 1) {
        const int r2 = rc == OK ? consume(slot) : OK;
        if (rc == OK) rc = r2;
    }
    if (rc != OK) (void)hipStreamSynchronize(st);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Batched range search: nq range queries against one index state.  The MFMA filter is a threshold
// filter, and for a range query the threshold is known before the first launch: the smallest bf16 key whose bound
// (score_bound.hpp, with the filter's in_extra) reaches min_score.  One pass of the shipped pass-1 kernel, then rescore /
// cut / rank / emit on the device; a query leaves this route only when its candidate buffer overflows, a score is NaN or
// more than RBATCH_SEG rows qualify -- then the single call answers it under the same lock.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr size_t RBATCH_SPEC = 65536;  // packed answer entries copied back with the counters (768 KB)
uint32_t range_batch_candidate_capacity()
{
    // VL_RANGE_BATCH_CAND_CAP: smaller per-query candidate buffers (tests drive the overflow route with it)
    if (const char* e = getenv("VL_RANGE_BATCH_CAND_CAP")) {
        const long long v = atoll(e);
        if (v >= 1 && v <= (long long)MFMA_CAND_CAP) return (uint32_t)v;
    }
    return (uint32_t)MFMA_CAND_CAP;
}
int ensure_range_batch_ws(Workspace* ws, uint64_t seq_queries)
{
    const size_t nq = MFMA_MAX_BATCH;
    VL_TRY(ensure_set(HipMem{}, {dev_buf(ws->rb_ctr, nq * RBATCH_CTR_WORDS), dev_buf(ws->rb_min, nq), pinned_buf(ws->rb_h_thr, nq),
                                 pinned_buf(ws->rb_h_min, nq), pinned_buf(ws->rb_h_ctr, nq * RBATCH_CTR_WORDS),
                                 pinned_buf(ws->rb_h_cnt, nq), pinned_buf(ws->rb_h_pos, RBATCH_SPEC),
                                 pinned_buf(ws->rb_h_scores, RBATCH_SPEC)}));
    // as many survivor segments as the largest sequence so far had queries
    return grow(HipMem{}, ws->rb_sv_queries, seq_queries,
                {dev_buf(ws->rb_sv_score, (size_t)seq_queries * RBATCH_SEG), dev_buf(ws->rb_sv_pos, (size_t)seq_queries * RBATCH_SEG)});
}
}  // namespace

int GpuFlatIndex::search_range_batch(uint64_t token, const double* queries, uint64_t nq, uint64_t q_len, const double* min_scores,
                                     int metric, uint64_t out_stride, uint64_t* out_ids, double* out_scores, uint64_t* out_n,
                                     uint64_t* out_total) const
{
    uint64_t routes[4] = {0, 0, 0, 0};  // MFMA route, single fast route, exact route; largest kept candidate count
    auto publish = [&]() {
        for (int i = 0; i < 4; ++i) last_rbatch_[i].store(routes[i], std::memory_order_relaxed);
    };
    if (nq == 0) {
        publish();
        return OK;
    }
    if (!out_n || !out_total || !min_scores) return ERR_INVALID_ARG;
    for (uint64_t i = 0; i < nq; ++i) {
        out_n[i] = 0;
        out_total[i] = 0;
    }
    std::shared_ptr<IdFilter> f;
    if (token != 0) VL_TRY(find_filter(token, &f));
    std::shared_lock<RwLock> lk;  // one index state for the whole batch
    VL_TRY(lock_for_query(metric, q_len, &lk));
    const uint64_t n = ids_.size();
    // The lowest failing query decides the status.  A NaN threshold fails its query before anything is computed, so only the
    // queries in front of the first one can fail earlier (with a NaN score): they are answered, the rest is not.
    uint64_t nq_run = nq;
    for (uint64_t i = 0; i < nq; ++i)
        if (min_scores[i] != min_scores[i]) {
            nq_run = i;
            break;
        }
    auto nan_threshold = [&]() -> int {
        set_last_error("min_score is NaN");
        return ERR_INVALID_ARG;
    };
    if (n == 0) {
        if (nq_run < nq) return nan_threshold();
        routes[1] = nq;
        publish();
        return OK;
    }
    if ((!queries && dim_) || (out_stride != 0 && !out_scores)) return ERR_INVALID_ARG;

    WsLease lease(this, /*sync_always=*/true);
    if (lease.status() != OK) return lease.status();
    Workspace* const ws = lease.ws;
    if (f) VL_TRY(resolve_if_stale(ws, f.get()));
    auto single = [&](uint64_t qi) -> int {
        if (f && f->m == 0) {  // an empty subset: nothing qualifies (search_range's early return)
            routes[1] += 1;
            return OK;
        }
        InFlight searching(active_searches_);
        const int rc = search_range_locked(ws, f.get(), queries + qi * dim_, min_scores[qi], metric, out_stride, nullptr,
                                           out_ids ? out_ids + qi * out_stride : nullptr,
                                           out_scores ? out_scores + qi * out_stride : nullptr, out_n + qi, out_total + qi);
        if (rc == OK) routes[last_path() == PATH_EXACT_SORT ? 2 : 1] += 1;
        return rc;
    };

    std::vector<uint8_t> done(nq_run, 0);
    const char* mf_env = getenv("VL_MFMA");
    const char* mf_min = getenv("VL_MFMA_MIN_BATCH");
    const uint64_t mfma_min = mf_min && *mf_min ? (uint64_t)atoi(mf_min) : (uint64_t)MFMA_MIN_BATCH;
    // (no minimum row count: the floor of the top-k batch belongs to its sampling pass, and this route has none)
    // The filter keeps `key >= thr`, which drops a NaN key, where the single scan's `!(key <= tau)` keeps it.  That is sound
    // only because NaN keys cannot occur on this route: rows outside the fast-path domain (n_out_of_domain_ != 0) take the
    // whole batch off it, and a query outside the domain is staged as zeros with thr = +inf and answered by the single call.
    const bool fast = !f && nq_run >= mfma_min && force_path_.load() == 0 && n_out_of_domain_ == 0 && !(mf_env && mf_env[0] == '0') &&
                      mfma_scan_supported((uint32_t)dim_, metric) && mfma_rows_kernel((uint32_t)dim_);
    if (fast) {
        VL_TRY(search_range_batch_mfma(ws, queries, nq_run, min_scores, metric, out_stride, out_ids, out_scores, out_n, out_total,
                                       &done, &routes[3]));
        for (uint64_t qi = 0; qi < nq_run; ++qi) routes[0] += done[qi] ? 1 : 0;
    }
    // what the MFMA route did not take (or everything), in ascending order: the first failure is the lowest failing query
    for (uint64_t qi = 0; qi < nq_run; ++qi)
        if (!done[qi]) VL_TRY(single(qi));
    if (nq_run < nq) return nan_threshold();
    set_last_path(routes[2] ? PATH_EXACT_SORT : PATH_FAST);
    publish();
    return OK;
}

int GpuFlatIndex::search_range_batch_mfma(Workspace* ws, const double* queries, uint64_t nq, const double* min_scores, int metric,
                                          uint64_t out_stride, uint64_t* out_ids, double* out_scores, uint64_t* out_n,
                                          uint64_t* out_total, std::vector<uint8_t>* done, uint64_t* max_candidates) const
{
    const uint64_t n = ids_.size();
    VL_TRY(ensure_bf16_slab(true));  // the row-stationary kernel's fragment-major slab, built as search_batch builds it
    VL_TRY(ensure_mfma_scratch(ws));
    const uint64_t seq = mfma_sequence_queries((uint32_t)dim_);
    VL_TRY(ensure_range_batch_ws(ws, std::min<uint64_t>(seq, nq)));
    hipStream_t st = ws->stream;
    const uint32_t ldb = mfma_ldb((uint32_t)dim_);
    const uint32_t cap = range_batch_candidate_capacity();
    const uint32_t emit_cap = (uint32_t)std::min<uint64_t>(out_stride, RBATCH_SEG);
    std::vector<uint8_t> staged;
    for (uint64_t q0 = 0; q0 < nq; q0 += seq) {
        const uint32_t g = (uint32_t)std::min<uint64_t>(seq, nq - q0);
        const size_t packed_cap = std::max<size_t>((size_t)g * emit_cap, 1);
        VL_TRY(ensure_range_ws(ws, 0, packed_cap));  // (allocates only while the stream is idle: every sequence ends in a sync)
        if (ws->mf_h2d_pending) {  // a top-k batch's copies out of the pinned staging area
            VL_HIP(hipEventSynchronize(ws->mf_ev_h2d));
            ws->mf_h2d_pending = false;
        }
        // stage: the queries as the top-k batch stages them, and per query the key threshold.  (R, Q) are the conventions of
        // that path's bound check: the index's largest row norm, the staged query norm, n = the bf16 row stride.
        staged.assign(g, 0);
        for (uint32_t j = 0; j < g; ++j) {
            double norm = 0.0;
            const bool in_domain = stage_query(queries + (q0 + j) * dim_, ws->mf_h_q64 + (size_t)j * dim_, dim_, &norm);
            float thr = INFINITY;  // no candidates: the query is peeled off to the single call, or nothing can qualify
            if (in_domain) {
                const RangeKeys r = range_key_threshold(metric, ldb, max_row_norm_, norm, min_scores[q0 + j], IN_EXTRA_MFMA, &thr);
                if (r == RANGE_KEYS_ALL) thr = INFINITY;  // every row a candidate (-inf, a zero query under cosine): not a filter's job
                else staged[j] = 1;
            }
            ws->rb_h_thr[j] = thr;
            ws->rb_h_min[j] = min_scores[q0 + j];
        }
        VL_HIP(hipMemcpyAsync(ws->mf_d_q64, ws->mf_h_q64, (size_t)g * dim_ * sizeof(double), hipMemcpyHostToDevice, st));
        VL_HIP(hipMemcpyAsync(ws->mf.thr, ws->rb_h_thr, (size_t)g * sizeof(float), hipMemcpyHostToDevice, st));
        VL_HIP(hipMemcpyAsync(ws->rb_min, ws->rb_h_min, (size_t)g * sizeof(double), hipMemcpyHostToDevice, st));
        VL_HIP(hipMemsetAsync(ws->rb_ctr, 0, (size_t)g * RBATCH_CTR_WORDS * sizeof(uint32_t), st));
        MfmaLaunchInfo li;
        VL_HIP(launch_mfma_range_candidates(st, metric, d_slab16f_, d_norm16_, d_sqnorm_, ws->mf_d_q64, g, n, (uint32_t)dim_, ws->mf,
                                            cap, &li));
        {
            const int v[6] = {li.ksteps, li.metric, li.chunks, li.grid_x, li.stages, li.sample_blocks};
            for (int i = 0; i < 6; ++i) last_filter_[i].store(v[i], std::memory_order_relaxed);
        }
        VL_HIP(launch_range_batch_tail(st, metric, ws->mf.cand, ws->mf.cnt, cap, g, d_master_, ws->mf_d_q64, ws->rb_min, (uint32_t)dim_,
                                       n, emit_cap, ws->rb_sv_score, ws->rb_sv_pos, ws->rb_ctr, ws->d_out_pos, ws->d_out_scores));
        // one copy back: counters, flags and the packed prefixes (as much of them as the speculative buffer holds)
        const size_t spec = std::min<size_t>((size_t)g * emit_cap, RBATCH_SPEC);
        VL_HIP(hipMemcpyAsync(ws->rb_h_ctr, ws->rb_ctr, (size_t)g * RBATCH_CTR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VL_HIP(hipMemcpyAsync(ws->rb_h_cnt, ws->mf.cnt, (size_t)g * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (spec) {
            VL_HIP(hipMemcpyAsync(ws->rb_h_pos, ws->d_out_pos, spec * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            VL_HIP(hipMemcpyAsync(ws->rb_h_scores, ws->d_out_scores, spec * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        VL_HIP(hipStreamSynchronize(st));

        // which queries the device answered, and how many packed entries that makes
        size_t packed = 0;
        for (uint32_t j = 0; j < g; ++j) {
            const uint32_t* c = ws->rb_h_ctr + (size_t)j * RBATCH_CTR_WORDS;
            const bool ok = staged[j] && ws->rb_h_cnt[j] <= cap && c[RBATCH_CTR_NAN] == 0 && c[RBATCH_CTR_TOTAL] <= RBATCH_SEG;
            if (!ok) {
                staged[j] = 0;
                continue;
            }
            const uint32_t want = (uint32_t)std::min<uint64_t>(c[RBATCH_CTR_TOTAL], emit_cap);
            if (c[RBATCH_CTR_TOTAL] > ws->rb_h_cnt[j] || c[RBATCH_CTR_WANT] != want || (size_t)c[RBATCH_CTR_OFF] + want > packed_cap) {
                set_last_error("batched range tail reported inconsistent counts (kernel bug)");
                return ERR_DEVICE;
            }
            packed = std::max(packed, (size_t)c[RBATCH_CTR_OFF] + want);
            if (max_candidates && ws->rb_h_cnt[j] > *max_candidates) *max_candidates = ws->rb_h_cnt[j];
        }
        std::vector<uint32_t> more_pos;
        std::vector<double> more_scores;
        if (packed > spec) {  // long answers: the rest of the packed prefixes
            more_pos.resize(packed - spec);
            more_scores.resize(packed - spec);
            VL_HIP(hipMemcpyAsync(more_pos.data(), ws->d_out_pos + spec, (packed - spec) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            VL_HIP(hipMemcpyAsync(more_scores.data(), ws->d_out_scores + spec, (packed - spec) * sizeof(double), hipMemcpyDeviceToHost,
                                  st));
            VL_HIP(hipStreamSynchronize(st));
        }
        for (uint32_t j = 0; j < g; ++j) {
            if (!staged[j]) continue;
            const uint64_t qi = q0 + j;
            const uint32_t* c = ws->rb_h_ctr + (size_t)j * RBATCH_CTR_WORDS;
            const size_t off = c[RBATCH_CTR_OFF];
            const uint32_t want = c[RBATCH_CTR_WANT];
            // packed entry e: in the speculative copy, or in the rest fetched behind it
            VL_TRY(deliver(
                "batched range search", ids_, want,
                [&](uint64_t i) { return off + i < spec ? ws->rb_h_pos[off + i] : more_pos[off + i - spec]; },
                [&](uint64_t i) { return off + i < spec ? ws->rb_h_scores[off + i] : more_scores[off + i - spec]; }, nullptr,
                out_ids ? out_ids + qi * out_stride : nullptr, out_scores + qi * out_stride));
            out_n[qi] = want;
            out_total[qi] = c[RBATCH_CTR_TOTAL];
            (*done)[qi] = 1;
        }
    }
    return OK;
}

// Queries in device memory.  The MFMA batch path takes them where they are; everything else goes through the host.
int GpuFlatIndex::search_batch_device(const double* d_queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric,
                                      uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n) const
{
    if (nq == 0) return OK;
    if (!out_n) return ERR_INVALID_ARG;
    for (uint64_t i = 0; i < nq; ++i) out_n[i] = 0;
    VL_TRY(check_metric(metric));
    VL_HIP(hipSetDevice(device_));
    auto via_host = [&]() -> int {  // the reference's surface with host queries: every check and path of search_batch()
        std::vector<double> h;
        if (d_queries && q_len) {
            try {
                h.resize((size_t)nq * q_len);
            } catch (const std::bad_alloc&) {
                set_last_error("out of host memory copying the queries");
                return ERR_OOM;
            }
            VL_HIP(hipMemcpy(h.data(), d_queries, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        return search_batch(d_queries ? h.data() : nullptr, nq, q_len, k, metric, out_pos, out_ids, out_scores, out_n);
    };
    std::shared_lock<RwLock> lk(mu_);
    const uint64_t n = ids_.size();
    // the checks of search_batch(), before any byte of the queries is touched (src/index/flat.rs:99-104: an empty index
    // accepts any query length)
    if (n != 0 && q_len != dim_) return dim_mismatch(q_len);
    if (n == 0 || k == 0) return OK;
    if (!d_queries || !out_scores) return ERR_INVALID_ARG;
    const uint64_t k_eff = std::min<uint64_t>(k, n);
    const char* mf_env = getenv("VL_MFMA");
    const char* mf_min = getenv("VL_MFMA_MIN_BATCH");
    const uint64_t mfma_min = mf_min && *mf_min ? (uint64_t)atoi(mf_min) : (uint64_t)MFMA_MIN_BATCH;
    const bool direct = nq > 1 && force_path_.load() == 0 &&
                        k_eff <= (uint64_t)KFAST_MAX && n_out_of_domain_ == 0 && !(mf_env && mf_env[0] == '0') &&
                        nq >= mfma_min && n >= MFMA_MIN_ROWS && mfma_scan_supported((uint32_t)dim_, metric);
    if (!direct) {
        lk.unlock();
        return via_host();
    }
    std::vector<uint8_t> done(nq, 0);
    {
        WsLease lease(this, /*sync_always=*/true);
        if (lease.status() != OK) return lease.status();
        VL_TRY(search_batch_mfma(lease.ws, nullptr, d_queries, nq, k, k_eff, metric, out_pos, out_ids, out_scores, out_n, &done));
    }
    set_last_path(PATH_FAST);
    // what the filter could not certify (ties, candidate overflow, a query outside the fast-path domain): those queries
    // go to the host and through search_batch(), results scattered back
    std::vector<uint64_t> left;
    for (uint64_t qi = 0; qi < nq; ++qi)
        if (!done[qi]) left.push_back(qi);
    if (left.empty()) return OK;
    const uint64_t m = left.size();
    std::vector<double> hq;
    std::vector<uint64_t> t_pos, t_ids, t_n;
    std::vector<double> t_sc;
    try {
        hq.resize(m * dim_);
        t_pos.resize(m * k_eff);
        t_ids.resize(m * k_eff);
        t_sc.resize(m * k_eff);
        t_n.resize(m);
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory answering the queries the MFMA filter could not certify");
        return ERR_OOM;
    }
    for (uint64_t i = 0; i < m; ++i)
        VL_HIP(hipMemcpy(hq.data() + i * dim_, d_queries + left[i] * dim_, dim_ * sizeof(double), hipMemcpyDeviceToHost));
    VL_TRY(search_batch_locked(hq.data(), m, dim_, k_eff, metric, t_pos.data(), t_ids.data(), t_sc.data(), t_n.data()));  // still under the caller's shared lock: one index state for the whole batch
    for (uint64_t i = 0; i < m; ++i) {
        const uint64_t qi = left[i];
        for (uint64_t j = 0; j < t_n[i]; ++j) {
            if (out_pos) out_pos[qi * k + j] = t_pos[i * k_eff + j];
            if (out_ids) out_ids[qi * k + j] = t_ids[i * k_eff + j];
            out_scores[qi * k + j] = t_sc[i * k_eff + j];
        }
        out_n[qi] = t_n[i];
    }
    return OK;
}

// ---------------------------------------------------------------------------------------------
// point lookups / export / clone
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::get_vector(uint64_t id, double* out) const
{
    if (!out && dim_) return ERR_INVALID_ARG;
    std::shared_lock<RwLock> lk(mu_);
    auto it = std::find(ids_.begin(), ids_.end(), id);  // first match (src/index/flat.rs:129-131)
    if (it == ids_.end()) return ERR_NOT_FOUND;
    const uint64_t pos = (uint64_t)(it - ids_.begin());
    if (dim_) {
        VL_HIP(hipSetDevice(device_));
        VL_HIP(hipMemcpy(out, d_master_ + pos * dim_, dim_ * sizeof(double), hipMemcpyDeviceToHost));
    }
    return OK;
}

int GpuFlatIndex::max_id(uint64_t* out) const
{
    if (!out) return ERR_INVALID_ARG;
    std::shared_lock<RwLock> lk(mu_);
    if (ids_.empty()) return ERR_NOT_FOUND;
    *out = *std::max_element(ids_.begin(), ids_.end());
    return OK;
}

int GpuFlatIndex::export_rows(uint64_t* out_ids, double* out_values) const
{
    std::shared_lock<RwLock> lk(mu_);
    const uint64_t n = ids_.size();
    if (n == 0) return OK;
    if (!out_ids || (!out_values && dim_)) return ERR_INVALID_ARG;
    std::memcpy(out_ids, ids_.data(), n * sizeof(uint64_t));
    if (dim_) {
        VL_HIP(hipSetDevice(device_));
        VL_HIP(hipMemcpy(out_values, d_master_, n * dim_ * sizeof(double), hipMemcpyDeviceToHost));
    }
    return OK;
}

int GpuFlatIndex::clone(GpuFlatIndex** out) const
{
    if (!out) return ERR_INVALID_ARG;
    *out = nullptr;
    std::shared_lock<RwLock> lk(mu_);
    GpuFlatIndex* c = nullptr;
    VL_TRY(create(dim_, device_, &c));
    std::unique_ptr<GpuFlatIndex> guard(c);
    if (!ids_.empty())
        VL_TRY(c->add_bulk(ids_.data(), d_master_, ids_.size(), /*validate=*/false, /*values_on_device=*/true));
    c->force_path_.store(force_path_.load());
    c->masked_batch_.store(masked_batch_.load());
    c->where_route_.store(where_route_.load());
    *out = guard.release();
    return OK;
}

// ---------------------------------------------------------------------------------------------
// HNSW distance callbacks (src/index/hnsw.rs:113-174)
// ---------------------------------------------------------------------------------------------
int GpuFlatIndex::hnsw_distances(const double* query, uint64_t q_len, int metric, const uint64_t* positions,
                                 uint64_t m, uint64_t* out) const
{
    if (metric < 0 || metric > 3) return ERR_INVALID_ARG;
    std::shared_lock<RwLock> lk(mu_);
    if (q_len != dim_) return dim_mismatch(q_len);
    if (m == 0) return OK;
    if (!positions || !out || (!query && dim_)) return ERR_INVALID_ARG;
    const uint64_t n = ids_.size();
    std::vector<uint32_t> p32(m);
    for (uint64_t i = 0; i < m; ++i) {
        if (positions[i] >= n) {
            set_last_error("position out of range");
            return ERR_NOT_FOUND;
        }
        p32[i] = (uint32_t)positions[i];
    }
    WsLease lease(this, /*sync_always=*/true);
    if (lease.status() != OK) return lease.status();
    Workspace* const ws = lease.ws;
    hipStream_t st = ws->stream;
    const size_t cap = std::max<size_t>(m, 256);
    VL_TRY(grow(HipMem{}, ws->hn_cap, cap, {dev_buf(ws->d_positions, cap), dev_buf(ws->d_dists, cap)}));
    for (uint64_t i = 0; i < dim_; ++i) ws->h_q64[i] = query[i];
    if (dim_) VL_HIP(hipMemcpyAsync(ws->d_q64, ws->h_q64, dim_ * sizeof(double), hipMemcpyHostToDevice, st));
    VL_HIP(hipMemcpyAsync(ws->d_positions, p32.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    VL_HIP(launch_hnsw_distances(st, metric, d_master_, ws->d_q64, (uint32_t)dim_, ws->d_positions, (uint32_t)m,
                                 ws->d_dists));
    VL_HIP(hipMemcpyAsync(out, ws->d_dists, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VL_HIP(hipStreamSynchronize(st));
    return OK;
}

// Ingest step in front of add (src/embeddings.rs:169-181): f32 embeddings are widened and
// normalised on the device in chunks (launch_embed_f32) and handed to `append` as device-resident f64 rows, so
// the host never holds an f64 copy and PCIe carries 4 bytes per value instead of 8.
int add_embeddings_f32(int device, uint64_t dim, const uint64_t* ids, const float* emb, uint64_t n, bool normalize,
                       bool emb_on_device, const std::function<int(const uint64_t*, const double*, uint64_t)>& append)
{
    if (n == 0) return OK;
    if (!ids || (!emb && dim)) return ERR_INVALID_ARG;
    VL_HIP(hipSetDevice(device));
    const uint64_t row_bytes = std::max<uint64_t>(dim, 1) * sizeof(double);
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(n, (512ull << 20) / row_bytes));
    struct Scratch {
        hipStream_t st = nullptr;
        double* rows = nullptr;
        float* staged = nullptr;
        ~Scratch()
        {
            if (rows) (void)hipFree(rows);
            if (staged) (void)hipFree(staged);
            if (st) (void)hipStreamDestroy(st);
        }
    } sc;
    VL_HIP(hipStreamCreateWithFlags(&sc.st, hipStreamNonBlocking));
    VL_HIP(hipMalloc(&sc.rows, chunk * row_bytes));
    if (!emb_on_device) VL_HIP(hipMalloc(&sc.staged, chunk * std::max<uint64_t>(dim, 1) * sizeof(float)));
    for (uint64_t done = 0; done < n; done += chunk) {
        const uint64_t c = std::min(chunk, n - done);
        const float* src = emb + done * dim;
        if (!emb_on_device && dim) {
            VL_HIP(hipMemcpyAsync(sc.staged, src, c * dim * sizeof(float), hipMemcpyHostToDevice, sc.st));
            src = sc.staged;
        }
        VL_HIP(launch_embed_f32(sc.st, src, c, (uint32_t)dim, normalize, sc.rows));
        VL_HIP(hipStreamSynchronize(sc.st));
        VL_TRY(append(ids + done, sc.rows, c));  // stops at the first duplicate id like n sequential add() calls
    }
    return OK;
}

int search_embeddings_f32(int device, uint64_t dim, const float* emb, uint64_t nq, bool normalize, bool emb_on_device,
                          const std::function<int(const double*, uint64_t)>& search)
{
    if (nq == 0) return OK;
    if (!emb && dim) return ERR_INVALID_ARG;
    if (dim == 0 || nq > (1ull << 31) / std::max<uint64_t>(dim, 1) * 64) {  // 16 GiB of f64 queries: not a batch
        set_last_error("query batch too large (or dimension 0)");
        return ERR_INVALID_ARG;
    }
    VL_HIP(hipSetDevice(device));
    // conversion scratch (a stream, the f64 queries, the staged f32 embeddings) comes from a small process-wide pool: a
    // hipMalloc / hipFree pair per call would cost more than the conversion kernel and synchronise the device
    struct Scratch {
        int device = 0;
        hipStream_t st = nullptr;
        double* rows = nullptr;
        size_t rows_cap = 0;
        float* staged = nullptr;
        size_t staged_cap = 0;
        ~Scratch()
        {
            (void)hipSetDevice(device);
            if (rows) (void)hipFree(rows);
            if (staged) (void)hipFree(staged);
            if (st) (void)hipStreamDestroy(st);
        }
    };
    static std::mutex pool_mu;
    static std::vector<std::unique_ptr<Scratch>> pool;  // idle scratches (at most 8 are kept)
    std::unique_ptr<Scratch> scp;
    {
        std::lock_guard<std::mutex> g(pool_mu);
        for (size_t i = 0; i < pool.size(); ++i)
            if (pool[i]->device == device) {
                scp = std::move(pool[i]);
                pool.erase(pool.begin() + (long)i);
                break;
            }
    }
    if (!scp) {
        scp.reset(new Scratch());
        scp->device = device;
        VL_HIP(hipStreamCreateWithFlags(&scp->st, hipStreamNonBlocking));
    }
    struct Return {
        std::unique_ptr<Scratch>& p;
        ~Return()
        {
            std::lock_guard<std::mutex> g(pool_mu);
            if (p && pool.size() < 8) pool.push_back(std::move(p));
        }
    } ret{scp};
    Scratch& sc = *scp;
    const size_t need = (size_t)nq * dim;
    VL_TRY(grow(HipMem{}, sc.rows_cap, need, {dev_buf(sc.rows, need)}));
    const float* src = emb;
    if (!emb_on_device) {
        VL_TRY(grow(HipMem{}, sc.staged_cap, need, {dev_buf(sc.staged, need)}));
        VL_HIP(hipMemcpyAsync(sc.staged, emb, need * sizeof(float), hipMemcpyHostToDevice, sc.st));
        src = sc.staged;
    }
    VL_HIP(launch_embed_f32(sc.st, src, nq, (uint32_t)dim, normalize, sc.rows));
    VL_HIP(hipStreamSynchronize(sc.st));
    return search(sc.rows, nq);
}

}  // namespace vl
