// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the distance-scan hot path.
//
// Reference semantics being reproduced (paths relative to /root/reference):
//   FlatIndex::search            src/index/flat.rs:98-119   (score every row, stable sort desc, truncate k)
//   SimilarityMetric::calculate  src/lib.rs:380-391, :425-572 (f64, strict index order, no FMA)
//   HNSW Metric::distance -> u64 src/index/hnsw.rs:113-174
//
// Design (DESIGN.md has the full argument):
//   * K1 k_scan: streams the [N, ld] f32 slab once. G lanes share a row, every lane issues 16-byte
//     non-temporal loads straight to VGPRs (no LDS round trip: nothing is reused), several row groups
//     in flight per wave; partial sums are reduced with cross-lane shuffles; each wave keeps a sorted
//     top-64 candidate list, ONE ENTRY PER LANE, updated by ballot/shuffle only when a row beats the
//     wave's current 64th key.  HBM-bound: 4*ld algorithmic bytes per row.
//   * K2 k_merge_finalize: merges the per-workgroup lists (bitonic merges in registers/LDS), then
//     RE-SCORES the 64 candidates from the f64 master rows in the reference's exact operation order
//     (separate multiply and add, index order, this file is compiled with -ffp-contract=off), ranks
//     them by (score desc, position asc) and proves -- with a rigorous f32 error bound on every row
//     that was NOT kept -- that no other row can reach the k-th score.  If the proof fails (ties at
//     the cut, adversarial data) the host re-runs the query on the exact kernels below.
//   * Exact path: k_exact_scan (reference-order f64 score of every row, LDS-transposed so global
//     reads stay coalesced) + k_select64 / bitonic sort on (score desc, position asc).
//   * k_hnsw_dist: the four HNSW distance callbacks, f64 reference order, Rust `as u64` semantics.
#include "kernels.hpp"
#include "device_common.hpp"
#include "scan_stream.hpp"
#include "score_bound.hpp"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <tuple>
#include <type_traits>

namespace vl {
using namespace dev;
static_assert(BOUND_COSINE == COSINE && BOUND_EUCLIDEAN == EUCLIDEAN && BOUND_MANHATTAN == MANHATTAN && BOUND_DOT == DOT,
              "score_bound.hpp carries the metric codes of kernels.hpp");
namespace {

// Merge level: workgroup (b, q) folds lists [64b, 64b+64) of query q (16 waves x 4 lists, then a
// 4-level tree) into one sorted list out[q][b].
template <typename K, typename C>
__global__ __launch_bounds__(1024) void k_merge_lists(const C* __restrict__ lists, int n_lists, size_t in_stride_q,
                                                      C* __restrict__ out, size_t out_stride_q)
{
    constexpr int NW = 16;
    __shared__ C sh[NW * WAVE];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    lists += (size_t)blockIdx.y * in_stride_q;
    out += (size_t)blockIdx.y * out_stride_q;
    const int first = blockIdx.x * 64 + wave * 4;
    int count = n_lists - first;
    count = count < 0 ? 0 : (count > 4 ? 4 : count);
    TopList<K> L;
    fold_lists4<K, C>(L, lists, first, count);
    block_merge<K, C, NW>(L, sh);
    if (wave == 0) {
        C e = {};
        e.key = L.key;
        e.pos = L.pos;
        out[(size_t)blockIdx.x * KP + lane] = e;
    }
}

// ---------------------------------------------------------------------------------------------
// K1: f32 slab scan
// ---------------------------------------------------------------------------------------------
template <int METRIC>
__device__ __forceinline__ float acc4(float a, const f32x4 x, const f32x4 q)
{
    if (METRIC == COSINE || METRIC == DOT) {
        a = fmaf(x.x, q.x, a);
        a = fmaf(x.y, q.y, a);
        a = fmaf(x.z, q.z, a);
        a = fmaf(x.w, q.w, a);
    } else if (METRIC == EUCLIDEAN) {
        const float d0 = x.x - q.x, d1 = x.y - q.y, d2 = x.z - q.z, d3 = x.w - q.w;
        a = fmaf(d0, d0, a);
        a = fmaf(d1, d1, a);
        a = fmaf(d2, d2, a);
        a = fmaf(d3, d3, a);
    } else {
        a += fabsf(x.x - q.x);
        a += fabsf(x.y - q.y);
        a += fabsf(x.z - q.z);
        a += fabsf(x.w - q.w);
    }
    return a;
}

// Scan key (larger = better) from the reduced row sum.  Cosine is ranked by dot * (1/|row|): the
// 1/|query| factor is the same positive number for every row.  Euclidean/Manhattan are ranked by
// the negated sum: 1/(1+sqrt(s)) and 1/(1+s) are monotone in s, so the scan needs no sqrt/division.
template <int METRIC>
__device__ __forceinline__ float scan_key(float sum, float inv_norm)
{
    if (METRIC == COSINE) return sum * inv_norm;
    if (METRIC == DOT) return sum;
    return -sum;
}

// The f32 slab as scan_stream()'s row format: a chunk is four columns, cosine carries 1/|row| with the row loads.
template <int METRIC, int VPL_>
struct F32Rows {
    typedef f32x4 Chunk;
    typedef f32x4 Query;
    typedef float Scalars;
    static constexpr int VPL = VPL_;
    const f32x4* __restrict__ slab;
    const float* __restrict__ inv_norm;
    __device__ __forceinline__ float load_scalars(uint32_t r) const
    {
        float inv = 1.0f;
        if (METRIC == COSINE) inv = inv_norm[r];
        return inv;
    }
    static __device__ __forceinline__ float accumulate(float a, const f32x4 x, const f32x4 q) { return acc4<METRIC>(a, x, q); }
    __device__ __forceinline__ float key(float sum, float inv) const { return scan_key<METRIC>(sum, inv); }
};

// K1, the single-query form: the f32 query travels IN THE KERNEL ARGUMENTS (rows of up to SCAN_QARG_FLOATS padded
// columns = 3 KB of the 4 KB kernarg segment), rounded on the host exactly as load_q4 rounds it here (f64 -> f32,
// nearest even).  No H2D copy precedes the scan: a search is this launch + the finalize kernel.
struct alignas(16) ScanQArg {
    float v[SCAN_QARG_FLOATS];
};

// The lane's slice of the f32 query (columns c + G j), from the kernel arguments ...
template <int G, int VPL>
__device__ __forceinline__ void load_query(f32x4 (&qv)[VPL], const ScanQArg& qa)
{
    static_assert(G * VPL * 4 <= SCAN_QARG_FLOATS, "row too long for the kernarg query");
    const int c = lane_id() % G;
#pragma unroll
    for (int j = 0; j < VPL; ++j) qv[j] = *reinterpret_cast<const f32x4*>(&qa.v[4 * (c + G * j)]);
}

// ... or from the f64 query in device memory (rows longer than the kernarg form holds; the multi-list k > 60 path,
// which stages the query on the device anyway).
template <int G, int VPL>
__device__ __forceinline__ void load_query(f32x4 (&qv)[VPL], const double* __restrict__ q64, uint32_t dim)
{
    const int c = lane_id() % G;
#pragma unroll
    for (int j = 0; j < VPL; ++j) qv[j] = load_q4(q64, c + G * j, dim);
}

// Specialised: ld4 == G * VPL float4 per row, U row groups in flight per wave.
template <int METRIC, int G, int VPL, int U>
__global__ __launch_bounds__(256) void k_scan(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                              uint32_t n, Cand32* __restrict__ out, const ScanQArg qa)
{
    f32x4 qv[VPL];
    load_query<G>(qv, qa);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, AllRows{}, n, TopSink(out));
}

template <int METRIC, int G, int VPL, int U>
__global__ __launch_bounds__(256) void k_scan_q64(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                  const double* __restrict__ q64, uint32_t dim, uint32_t n,
                                                  Cand32* __restrict__ out)
{
    f32x4 qv[VPL];
    load_query<G>(qv, q64, dim);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, AllRows{}, n, TopSink(out));
}

// K1 under an exclusion filter's keep bitmap: every row is streamed and scored as in k_scan, a row
// whose bit is 0 is never offered.  Compiled for the default shape of each stride (k_scan_subset's rule): the query in the
// kernel arguments, or -- strides past the kernel-argument query -- the f64 query in device memory (k_scan_q64's form).
template <int METRIC, int G, int VPL, int U>
__global__ __launch_bounds__(256) void k_scan_masked(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                     const unsigned long long* __restrict__ keep, uint32_t n,
                                                     Cand32* __restrict__ out, const ScanQArg qa)
{
    f32x4 qv[VPL];
    load_query<G>(qv, qa);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, MaskedRows{keep}, n, TopSink(out));
}

template <int METRIC, int G, int VPL, int U>
__global__ __launch_bounds__(256) void k_scan_masked_q64(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                         const unsigned long long* __restrict__ keep,
                                                         const double* __restrict__ q64, uint32_t dim, uint32_t n,
                                                         Cand32* __restrict__ out)
{
    f32x4 qv[VPL];
    load_query<G>(qv, q64, dim);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, MaskedRows{keep}, n, TopSink(out));
}

// Generic: any ld4 (float4 per row), G = lanes per row (power of two <= 64), one row group per step, the query read
// as it is needed.  scan_stream()'s row sources and sinks; the same acc4 column order, group_reduce and scan_key, so a
// row's key does not depend on which of the three families scores it.  A listed row's entry for the NEXT step is
// requested before this step's row is read.
template <int METRIC, int G, class Rows, class Sink>
__device__ __forceinline__ void scan_stream_generic(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                    const double* __restrict__ q64, uint32_t dim, uint32_t n, uint32_t ld4,
                                                    const Rows rows, Sink sink)
{
    constexpr int RPS = WAVE / G;
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int g = lane / G, c = lane % G;
    const uint32_t n_steps = (n + RPS - 1) / RPS;
    const uint32_t n_waves = gridDim.x * 4;

    uint32_t s = blockIdx.x * 4 + wave;
    uint32_t i_next = s < n_steps ? s * RPS + g : n;  // n marks "no row"
    uint32_t p_next = rows.at(i_next, n);
    for (; s < n_steps; s += n_waves) {
        const bool valid = i_next < n;
        const uint32_t pos = p_next;
        const uint32_t sn = s + n_waves;
        i_next = sn < n_steps ? sn * RPS + g : n;
        p_next = rows.at(i_next, n);
        const uint32_t r = rows.load_row(pos, valid, n);
        const f32x4* p = slab + (size_t)r * ld4;
        float a = 0.0f;
        for (uint32_t j = c; j < ld4; j += G) a = acc4<METRIC>(a, p[j], load_q4(q64, j, dim));
        a = group_reduce<G>(a);
        float inv = 1.0f;
        if (METRIC == COSINE) inv = inv_norm[r];
        sink.offer(0, scan_key<METRIC>(a, inv), pos, valid && c == 0);
        sink.step();
    }
    sink.finish();
}

template <int METRIC, int G>
__global__ __launch_bounds__(256) void k_scan_generic(const f32x4* __restrict__ slab,
                                                      const float* __restrict__ inv_norm,
                                                      const double* __restrict__ q64, uint32_t dim, uint32_t n,
                                                      uint32_t ld4, Cand32* __restrict__ out)
{
    scan_stream_generic<METRIC, G>(slab, inv_norm, q64, dim, n, ld4, AllRows{}, TopSink(out));
}

// K1 over a subset: the rows are plist[0..m) (ascending storage positions, an id filter's resolution).  The list
// entries carry STORAGE positions and reach the sink in ascending order within each wave's stream, as in k_scan.
// The kernel-argument query (k_scan's form) ...
template <int METRIC, int G, int VPL, int U>
__global__ __launch_bounds__(256) void k_scan_subset(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                     const uint32_t* __restrict__ plist, uint32_t m, Cand32* __restrict__ out,
                                                     const ScanQArg qa)
{
    f32x4 qv[VPL];
    load_query<G>(qv, qa);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, ListedRows{plist}, m, TopSink(out));
}

// ... and the f64 query in device memory (k_scan_q64's form: strides past the kernarg query)
template <int METRIC, int G, int VPL, int U>
__global__ __launch_bounds__(256) void k_scan_subset_q64(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                         const uint32_t* __restrict__ plist, const double* __restrict__ q64,
                                                         uint32_t dim, uint32_t m, Cand32* __restrict__ out)
{
    f32x4 qv[VPL];
    load_query<G>(qv, q64, dim);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, ListedRows{plist}, m, TopSink(out));
}

template <int METRIC, int G>
__global__ __launch_bounds__(256) void k_scan_subset_generic(const f32x4* __restrict__ slab,
                                                             const float* __restrict__ inv_norm,
                                                             const uint32_t* __restrict__ plist,
                                                             const double* __restrict__ q64, uint32_t dim, uint32_t m,
                                                             uint32_t ld4, Cand32* __restrict__ out)
{
    scan_stream_generic<METRIC, G>(slab, inv_norm, q64, dim, m, ld4, ListedRows{plist}, TopSink(out));
}

// K1 over MANY subsets in one launch: blockIdx.y is the job, jobs[job] names its list, its f64 query is row `job` of q64
// (load_query's device form: the rounding of the kernel-argument form, so a row's key is k_scan_subset's bit for bit).
// Every job has gridDim.x workgroups; scan_stream strides by gridDim.x and TopSink writes list blockIdx.x of the job's
// gridDim.x lists, so the skeleton is k_scan_subset's.  A workgroup with no step for its job writes the empty list.
template <int METRIC, int G, int VPL, int U>
__global__ __launch_bounds__(256) void k_scan_subset_jobs(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                          const SubsetJobDev* __restrict__ jobs, const double* __restrict__ q64,
                                                          uint32_t dim, Cand32* __restrict__ out)
{
    const SubsetJobDev job = jobs[blockIdx.y];
    f32x4 qv[VPL];
    load_query<G>(qv, q64 + (size_t)blockIdx.y * dim, dim);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, ListedRows{job.plist}, job.m,
                      TopSink(out + (size_t)blockIdx.y * gridDim.x * KP));
}

template <int METRIC, int G>
__global__ __launch_bounds__(256) void k_scan_subset_jobs_generic(const f32x4* __restrict__ slab,
                                                                  const float* __restrict__ inv_norm,
                                                                  const SubsetJobDev* __restrict__ jobs,
                                                                  const double* __restrict__ q64, uint32_t dim, uint32_t ld4,
                                                                  Cand32* __restrict__ out)
{
    const SubsetJobDev job = jobs[blockIdx.y];
    scan_stream_generic<METRIC, G>(slab, inv_norm, q64 + (size_t)blockIdx.y * dim, dim, job.m, ld4, ListedRows{job.plist},
                                   TopSink(out + (size_t)blockIdx.y * gridDim.x * KP));
}

// Resolution of an id filter: which storage positions hold an id of the sorted, deduplicated set fids[0..nf).  Workgroup b
// owns positions [b chunk, (b+1) chunk); pass 1 counts its matches, one workgroup turns the counts into offsets (and m), pass 2
// writes the matching positions of each chunk in ascending order at its offset: the list comes out ascending.
// `invert` (an exclusion filter): a position qualifies iff its id is NOT in the set; nf may then be 0 (fids is not read).
__device__ __forceinline__ bool id_in_set(unsigned long long id, const unsigned long long* __restrict__ fids, uint32_t nf)
{
    uint32_t lo = 0, hi = nf;  // lower_bound
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (fids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < nf && fids[lo] == id;
}

constexpr int FILTER_MAX_GRID = FILTER_COUNTS_MAX;

__global__ __launch_bounds__(256) void k_filter_count(const unsigned long long* __restrict__ pos_ids, uint32_t n,
                                                      const unsigned long long* __restrict__ fids, uint32_t nf,
                                                      uint32_t chunk, uint32_t* __restrict__ counts, uint32_t invert)
{
    __shared__ uint32_t sh_cnt[4];
    const uint32_t lo = blockIdx.x * chunk;
    const uint32_t hi = (uint64_t)lo + chunk < n ? lo + chunk : n;
    uint32_t cnt = 0;
    for (uint32_t p = lo + threadIdx.x; p < hi; p += 256) cnt += (id_in_set(pos_ids[p], fids, nf) != (invert != 0)) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane_id() == 0) sh_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
}

// exclusive scan of the nb <= FILTER_MAX_GRID counts in place; total -> *m_out
__global__ __launch_bounds__(FILTER_MAX_GRID) void k_filter_scan(uint32_t* __restrict__ counts, uint32_t nb,
                                                                 uint32_t* __restrict__ m_out)
{
    __shared__ uint32_t sh[FILTER_MAX_GRID];
    const uint32_t t = threadIdx.x;
    sh[t] = t < nb ? counts[t] : 0u;
    __syncthreads();
    for (uint32_t o = 1; o < FILTER_MAX_GRID; o <<= 1) {  // Hillis-Steele inclusive scan
        const uint32_t v = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    if (t < nb) counts[t] = t ? sh[t - 1] : 0u;
    if (t == FILTER_MAX_GRID - 1) *m_out = sh[t];
}

__global__ __launch_bounds__(256) void k_filter_compact(const unsigned long long* __restrict__ pos_ids, uint32_t n,
                                                        const unsigned long long* __restrict__ fids, uint32_t nf,
                                                        uint32_t chunk, const uint32_t* __restrict__ offsets,
                                                        uint32_t m_cap, uint32_t* __restrict__ plist, uint32_t invert)
{
    __shared__ uint32_t sh_cnt[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t lo = blockIdx.x * chunk;
    const uint32_t hi = (uint64_t)lo + chunk < n ? lo + chunk : n;
    uint32_t base = offsets[blockIdx.x];
    for (uint32_t t0 = lo; t0 < hi; t0 += 256) {  // block-uniform trip count
        const uint32_t p = t0 + threadIdx.x;
        const bool hit = p < hi && (id_in_set(pos_ids[p], fids, nf) != (invert != 0));
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) sh_cnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += sh_cnt[w];
        const uint32_t total = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
        const uint32_t rank = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (hit && base + rank < m_cap) plist[base + rank] = p;
        base += total;
        __syncthreads();  // sh_cnt is rewritten by the next tile
    }
}

// The keep bitmap of an exclusion filter: bit p & 63 of keep[p >> 6] is set iff p < n and ids[p] is NOT in the set.  One
// wave per word: the 64 lanes ballot their rows' membership, lane 0 stores the inverted word (bits at or past n are 0).
// include != 0 (an include token's rows): the word itself, bit set iff ids[p] IS in the set.
__global__ __launch_bounds__(256) void k_filter_bits(const unsigned long long* __restrict__ pos_ids, uint32_t n,
                                                     const unsigned long long* __restrict__ fids, uint32_t nf,
                                                     uint32_t n_words, unsigned long long* __restrict__ keep, uint32_t include)
{
    const int lane = lane_id();
    const uint32_t n_waves = gridDim.x * 4;
    for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < n_words; w += n_waves) {  // wave-uniform trip count
        const uint32_t p = w * 64u + (uint32_t)lane;
        const bool there = p < n;
        const bool in_set = there && id_in_set(pos_ids[p], fids, nf);
        const unsigned long long in_word = __ballot(in_set);
        const unsigned long long word = include ? in_word : (__ballot(there) & ~in_word);
        if (lane == 0) keep[w] = word;
    }
}

// ---------------------------------------------------------------------------------------------
// Range search: the f32 scan with RangeSink in the TopList's place, over every row or
// (SUBSET) over plist[0..n).  A row's key is bit for bit the one k_scan gives it.
// ---------------------------------------------------------------------------------------------
template <bool SUBSET>
__device__ __forceinline__ auto range_rows(const uint32_t* __restrict__ plist)
{
    if constexpr (SUBSET) return ListedRows{plist};
    else return AllRows{};
}

// the kernel-argument query (k_scan's form)
template <int METRIC, int G, int VPL, int U, bool SUBSET>
__global__ __launch_bounds__(256) void k_scan_range(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                    const uint32_t* __restrict__ plist, uint32_t n, float tau,
                                                    uint32_t* __restrict__ cand, uint32_t cap, uint32_t* __restrict__ ctr,
                                                    const ScanQArg qa)
{
    f32x4 qv[VPL];
    load_query<G>(qv, qa);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, range_rows<SUBSET>(plist), n, RangeSink<U>(tau, cand, cap, ctr));
}

// the f64 query in device memory (k_scan_q64's form: strides past the kernarg query)
template <int METRIC, int G, int VPL, int U, bool SUBSET>
__global__ __launch_bounds__(256) void k_scan_range_q64(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                        const uint32_t* __restrict__ plist,
                                                        const double* __restrict__ q64, uint32_t dim, uint32_t n, float tau,
                                                        uint32_t* __restrict__ cand, uint32_t cap,
                                                        uint32_t* __restrict__ ctr)
{
    f32x4 qv[VPL];
    load_query<G>(qv, q64, dim);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, range_rows<SUBSET>(plist), n, RangeSink<U>(tau, cand, cap, ctr));
}

template <int METRIC, int G, bool SUBSET>
__global__ __launch_bounds__(256) void k_scan_range_generic(const f32x4* __restrict__ slab,
                                                            const float* __restrict__ inv_norm,
                                                            const uint32_t* __restrict__ plist,
                                                            const double* __restrict__ q64, uint32_t dim, uint32_t n,
                                                            uint32_t ld4, float tau, uint32_t* __restrict__ cand,
                                                            uint32_t cap, uint32_t* __restrict__ ctr)
{
    scan_stream_generic<METRIC, G>(slab, inv_norm, q64, dim, n, ld4, range_rows<SUBSET>(plist), RangeSink<1>(tau, cand, cap, ctr));
}

// ---------------------------------------------------------------------------------------------
// Grouped search, pass 1: the f32 scan with GroupBestSink, over every row or (SUBSET) over
// plist[0..n).  A row's key is bit for bit the one k_scan gives it.  The three forms of the range scan.
// ---------------------------------------------------------------------------------------------
template <int METRIC, int G, int VPL, int U, bool SUBSET>
__global__ __launch_bounds__(256) void k_scan_group_best(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                         const uint32_t* __restrict__ plist, uint32_t n,
                                                         const uint32_t* __restrict__ group_of_row,
                                                         unsigned long long* __restrict__ best, const ScanQArg qa)
{
    f32x4 qv[VPL];
    load_query<G>(qv, qa);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, range_rows<SUBSET>(plist), n, GroupBestSink<U>(group_of_row, best));
}

template <int METRIC, int G, int VPL, int U, bool SUBSET>
__global__ __launch_bounds__(256) void k_scan_group_best_q64(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                             const uint32_t* __restrict__ plist,
                                                             const double* __restrict__ q64, uint32_t dim, uint32_t n,
                                                             const uint32_t* __restrict__ group_of_row,
                                                             unsigned long long* __restrict__ best)
{
    f32x4 qv[VPL];
    load_query<G>(qv, q64, dim);
    scan_stream<G, U>(F32Rows<METRIC, VPL>{slab, inv_norm}, qv, range_rows<SUBSET>(plist), n, GroupBestSink<U>(group_of_row, best));
}

template <int METRIC, int G, bool SUBSET>
__global__ __launch_bounds__(256) void k_scan_group_best_generic(const f32x4* __restrict__ slab,
                                                                 const float* __restrict__ inv_norm,
                                                                 const uint32_t* __restrict__ plist,
                                                                 const double* __restrict__ q64, uint32_t dim, uint32_t n,
                                                                 uint32_t ld4, const uint32_t* __restrict__ group_of_row,
                                                                 unsigned long long* __restrict__ best)
{
    scan_stream_generic<METRIC, G>(slab, inv_norm, q64, dim, n, ld4, range_rows<SUBSET>(plist), GroupBestSink<1>(group_of_row, best));
}

// K3: small-batch scan.  One pass over the slab serves QB queries: each row group is loaded ONCE into
// registers and scored against QB queries whose f32 copies sit in LDS (lanes that share a column read
// the same 16 bytes: an LDS broadcast).  Per wave, QB independent top-64 lists.  Still streams
// N*ld*4 bytes per pass; with QB = 8 the f32 VALU work (2*QB flop per 4 bytes) is about level with
// the HBM time, beyond that the GEMM/MFMA form takes over.
template <int METRIC, int G, int VPL, int QB>
__global__ __launch_bounds__(256) void k_scan_batch(const f32x4* __restrict__ slab, const float* __restrict__ inv_norm,
                                                    const double* __restrict__ q64, uint32_t n_q, uint32_t dim,
                                                    uint32_t n, Cand32* __restrict__ out)
{
    constexpr int RPS = WAVE / G;
    constexpr uint32_t LD4 = G * VPL;
    __shared__ f32x4 qs[QB][LD4];
    __shared__ Cand32 sh[4 * WAVE];
    // Lazy insertion (round 4).  A row that beats a list's 64th entry is not inserted at once (ballot, rank, two DPP shifts,
    // selects: ~25 dependent instructions per entry, and on a SMALL index every wave builds its lists from the ~1 500 rows it
    // sees -- 64 (1 + ln(rows / 64)) ~ 270 insertions per list: 69 % of this kernel on a 50 000-row index, measured with the
    // insertions compiled out): it is appended to a 64-entry buffer of its (wave, query) in LDS, and a full buffer is sorted
    // (bitonic, registers) and merged into the list in one go -- ~4 instructions per entry.  The threshold the rows are held
    // against is a little stale in between (more rows pass than would one by one); nothing that belongs is ever dropped, and
    // the list after a merge is the top 64 of everything the wave has seen: the same lists as before, bit for bit.
    __shared__ Cand32 cbuf[4][QB][WAVE];
    // qs + sh + cbuf, static: 67 584 B for the widest shape (16 lanes x 24 chunks, stride 1536).  That is past the 64 KB a
    // workgroup gets on every CDNA part before gfx950 (160 KB): this build is gfx950-only.
    static_assert(sizeof(f32x4) * QB * LD4 + sizeof(Cand32) * 4 * WAVE + sizeof(Cand32) * 4 * QB * WAVE <= 160u * 1024u,
                  "k_scan_batch: static LDS of this shape exceeds a gfx950 workgroup's 160 KB");

    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int g = lane / G, c = lane % G;
    // blockIdx.y = a group of QB queries: groups share nothing but the slab (one launch answers up to gridDim.y * QB queries;
    // on a small index that is what keeps the chip busy -- one group's pass is a few workgroups)
    {
        const uint32_t first = blockIdx.y * QB;
        q64 += (size_t)first * dim;
        out += (size_t)first * gridDim.x * KP;
        n_q = n_q - first < (uint32_t)QB ? n_q - first : (uint32_t)QB;
    }

    for (uint32_t idx = threadIdx.x; idx < QB * LD4; idx += 256) {
        const uint32_t qi = idx / LD4, j = idx % LD4;
        f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        qs[qi][j] = qi < n_q ? load_q4(q64 + (size_t)qi * dim, j, dim) : z;
    }
    __syncthreads();

    const uint32_t n_steps = (n + RPS - 1) / RPS;
    const uint32_t n_waves = gridDim.x * 4;

    TopList<float> L[QB];
    uint32_t n_buf[QB];  // wave-uniform: entries waiting in cbuf[wave][qi]
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
        L[qi].init();
        n_buf[qi] = 0;
    }
    auto flush = [&](int qi) {  // cbuf[wave][qi][0 .. n_buf) -> sorted -> merged into L[qi]
        float fk = -INFINITY;
        uint32_t fp = POS_SENTINEL;
        asm volatile("" : "+v"(fk));  // (keeps the -inf out of constant propagation, as in TopList::init)
        if ((uint32_t)lane < n_buf[qi]) {
            const Cand32 e = cbuf[wave][qi][lane];
            fk = e.key;
            fp = e.pos;
        }
        sort64_reversed<float>(fk, fp);
        L[qi].merge_reversed(fk, fp);
        n_buf[qi] = 0;
    };

    for (uint32_t s = blockIdx.x * 4 + wave; s < n_steps; s += n_waves) {
        const uint32_t row = s * RPS + g;
        const bool valid = row < n;
        const uint32_t r = valid ? row : n - 1;
        const f32x4* p = slab + (size_t)r * LD4 + c;
        f32x4 x[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) x[j] = __builtin_nontemporal_load(p + G * j);
        float inv = 1.0f;
        if (METRIC == COSINE) inv = inv_norm[r];
#pragma unroll
        for (int qi = 0; qi < QB; ++qi) {
            float a = 0.0f;
#pragma unroll
            for (int j = 0; j < VPL; ++j) a = acc4<METRIC>(a, x[j], qs[qi][c + G * j]);
            a = group_reduce<G>(a);
#ifndef VL_DBG_K3_NOINSERT
            {
                const float key = scan_key<METRIC>(a, inv);
                const bool cand = valid && c == 0 && (uint32_t)qi < n_q && better<float>(key, row, L[qi].thr_key, L[qi].thr_pos);
                const unsigned long long m = __ballot(cand);
                if (m != 0ull) {  // wave-uniform; at most RPS lanes offer a row per step
                    const uint32_t slot = n_buf[qi] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (cand) {
                        Cand32 e;
                        e.key = key;
                        e.pos = row;
                        cbuf[wave][qi][slot] = e;
                    }
                    n_buf[qi] += (uint32_t)__popcll(m);
                    if (n_buf[qi] > (uint32_t)(WAVE - RPS)) flush(qi);  // the next step could overflow the buffer
                }
            }
#else  // diagnostic build (tools/build_variant_k.sh): what does the scan cost WITHOUT the top-64 list maintenance?
            if (scan_key<METRIC>(a, inv) == 12345.678f) L[qi].pos = row;
#endif
            // one query's LDS reads at a time: without this the scheduler hoists every query's
            // 48 registers of LDS loads above the first FMA and the kernel needs 460+ VGPRs
            __builtin_amdgcn_sched_barrier(0);
        }
    }

#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
        if ((uint32_t)qi < n_q) {  // uniform
            if (n_buf[qi]) flush(qi);
            block_merge<float, Cand32, 4>(L[qi], sh);
            if (wave == 0) {
                Cand32 e;
                e.key = L[qi].key;
                e.pos = L[qi].pos;
                out[((size_t)qi * gridDim.x + blockIdx.x) * KP + lane] = e;
            }
            __syncthreads();
        }
    }
}

// Rescore up to 64 rows (positions in LDS) against the query: global reads are coalesced along the
// row (all threads load a [64][CH] f64 tile into LDS), then lanes 0..63 of wave 0 each walk one
// row's chunk in index order.  Row stride CH+1 doubles keeps the per-lane ds_read_b64 conflict-free.
constexpr int RESCORE_CH = 96;

template <int METRIC, int NTHREADS>
__device__ __forceinline__ void rescore_rows(const double* __restrict__ master, const double* __restrict__ q64,
                                             uint32_t dim, const uint32_t* sh_pos, int n_rows,
                                             double (*tile)[RESCORE_CH + 1], double* qtile, Acc64<METRIC>& A)
{
    // PF chunks of 96 columns are fetched from HBM together (one memory latency for 384 columns
    // instead of four); they then pass through the LDS tile one after the other, in column order.
    constexpr int PER = (KP * RESCORE_CH + NTHREADS - 1) / NTHREADS;  // tile elements per thread
    constexpr int PF = (NTHREADS >= 1024) ? 4 : 1;
    const int tid = threadIdx.x;
    A.init();
    if (n_rows <= 0) return;  // workgroup-uniform (an all-sentinel candidate list)
    for (uint32_t g0 = 0; g0 < dim; g0 += PF * RESCORE_CH) {
        double pre[PF][PER];
        double qpre[PF];
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const uint32_t c0 = g0 + p * RESCORE_CH;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                // clamped, never predicated (a load under a condition is waited for before the next one issues):
                // rows >= n_rows are not walked and columns >= dim not stepped, so the duplicates are unused
                int idx = tid + i * NTHREADS;
                idx = idx < KP * RESCORE_CH ? idx : KP * RESCORE_CH - 1;
                int r = idx / RESCORE_CH;
                r = r < n_rows ? r : n_rows - 1;
                uint32_t col = c0 + (uint32_t)(idx % RESCORE_CH);
                col = col < dim ? col : dim - 1;
                pre[p][i] = master[(size_t)sh_pos[r] * dim + col];
            }
            {
                uint32_t col = c0 + (uint32_t)(tid % RESCORE_CH);
                col = col < dim ? col : dim - 1;
                qpre[p] = q64[col];
            }
        }
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const uint32_t c0 = g0 + p * RESCORE_CH;
            if (c0 >= dim) break;  // workgroup-uniform
            const uint32_t cw = (dim - c0) < (uint32_t)RESCORE_CH ? (dim - c0) : (uint32_t)RESCORE_CH;
            __syncthreads();  // previous chunk fully consumed
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int idx = tid + i * NTHREADS;
                if (idx < KP * RESCORE_CH) tile[idx / RESCORE_CH][idx % RESCORE_CH] = pre[p][i];
            }
            if (tid < RESCORE_CH) qtile[tid] = qpre[p];
            __syncthreads();
            if (tid < n_rows) {
                uint32_t cc = 0;
                for (; cc + 8 <= cw; cc += 8) {  // 16 LDS reads in flight, then 8 steps in index order
                    double xv[8], yv[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        xv[t] = tile[tid][cc + t];
                        yv[t] = qtile[cc + t];
                    }
#pragma unroll
                    for (int t = 0; t < 8; ++t) A.step(xv[t], yv[t]);
                }
                for (; cc < cw; ++cc) A.step(tile[tid][cc], qtile[cc]);
            }
        }
    }
}

#ifdef VL_DBG_STAMPS
// diagnostic build only (tools/build_variant_k.sh): 100 MHz timestamps of the phases of one finalize launch
__device__ unsigned long long vl_dbg_stamps[32];
#define VL_STAMP(i)                                                                  \
    do {                                                                             \
        if (threadIdx.x == 0 && blockIdx.x == 0) {                                   \
            vl_dbg_stamps[i] = __builtin_amdgcn_s_memrealtime();                     \
            vl_dbg_stamps[16 + (i)] = __builtin_amdgcn_s_memtime(); /* shader clock */ \
        }                                                                            \
    } while (0)
#else
#define VL_STAMP(i) do {} while (0)
#endif

// The finalize kernels' rescoring (1024 threads): the same reference arithmetic with the serial part cut down to
// what the reference makes serial.  `a += x * y` under -ffp-contract=off is t = fl(x * y); a = fl(a + t): the
// products do not depend on the running sum, so ALL threads compute them while they move the rows through LDS
// (64 rows x 48 columns per tile), and one lane per row then only ADDS them in index order.  Cosine's three sums
// (x.y, x.x, y.y) are walked by three different waves at the same time.  Per row that leaves `dim` dependent f64
// adds (~2 us at dim 384) where rescore_rows walks dim x (2 LDS reads + 6 dependent f64 operations).
constexpr int RP_CH = 48;               // columns per LDS tile (row stride 49 doubles: conflict-free ds_read_b64)
constexpr int RP_NCH = 8;               // tiles per block of columns fetched from HBM together
constexpr int RP_BW = RP_CH * RP_NCH;   // 384 columns: one memory round trip for a dim-384 row

template <int METRIC, int ROWS = KP, int NCH = RP_NCH>
struct RescoreLds {
    double tA[ROWS][RP_CH + 1];                                 // the summands of `a`
    double tB[METRIC == COSINE ? ROWS : 1][RP_CH + 1];          // cosine: x * x
    double qblk[RP_CH * NCH];                                   // the query's columns of the current block
    double qq[METRIC == COSINE ? RP_CH * NCH : 1];              // cosine: y * y
    double b[ROWS];
    double c;
};

// ROWS candidate rows rescored by a workgroup of NTHREADS threads (ROWS * RP_CH tile elements, RP_PER per thread):
// 64 rows x 1024 threads for a single search's finalize, 16 rows x 256 threads for a quarter of a batch query's list.
template <int METRIC, int ROWS, int NTHREADS, int NCH = RP_NCH>
__device__ __forceinline__ void rescore_rows_par(const double* __restrict__ master, const double* __restrict__ q64,
                                                 uint32_t dim, const uint32_t* sh_pos, int n_rows,
                                                 RescoreLds<METRIC, ROWS, NCH>& S, Acc64<METRIC>& A,
                                                 const double (&q_first)[(RP_CH * NCH + NTHREADS - 1) / NTHREADS])
{
    // q_first[j]: q64[min(tid + j NTHREADS, dim - 1)], fetched by the caller at kernel entry (a single search reads
    // its query from pinned host memory: that PCIe round trip then hides behind the list merge)
    constexpr int RP_PER = ROWS * RP_CH / NTHREADS;
    constexpr int BW = RP_CH * NCH;  // columns fetched from HBM together (one memory round trip)
    constexpr int QN = (BW + NTHREADS - 1) / NTHREADS;
    static_assert(ROWS * RP_CH % NTHREADS == 0 && ROWS <= WAVE, "tile elements divide evenly; one lane per row");
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1), wave = tid >> 6;
    A.init();
    if (n_rows <= 0) return;  // workgroup-uniform (an all-sentinel candidate list)
    // what this thread accumulates: wave 0 the rows' `a`, wave 1 their `b`, wave 2 the query's `c` (cosine)
    double acc = (METRIC == COSINE) ? 0.0 : -0.0;
    for (uint32_t g0 = 0; g0 < dim; g0 += BW) {
        double pre[NCH][RP_PER];
#pragma unroll
        for (int p = 0; p < NCH; ++p) {
            const uint32_t c0 = g0 + p * RP_CH;
#pragma unroll
            for (int i = 0; i < RP_PER; ++i) {
                // clamped, never predicated (a load under a condition is waited for before the next one issues):
                // rows >= n_rows are not walked and columns >= dim not summed, so the duplicates are unused
                const int idx = tid + i * NTHREADS;
                int r = idx / RP_CH;
                r = r < n_rows ? r : n_rows - 1;
                uint32_t col = c0 + (uint32_t)(idx % RP_CH);
                col = col < dim ? col : dim - 1;
                pre[p][i] = master[(size_t)sh_pos[r] * dim + col];
            }
        }
        double qv[QN];
#pragma unroll
        for (int j = 0; j < QN; ++j) {
            qv[j] = q_first[j];
            if (g0 != 0 && tid + j * NTHREADS < BW) {
                const uint32_t col = g0 + (uint32_t)(tid + j * NTHREADS);
                qv[j] = q64[col < dim ? col : dim - 1];
            }
        }
        VL_STAMP(4);
        __syncthreads();  // the previous block's qblk / tiles are consumed
#pragma unroll
        for (int j = 0; j < QN; ++j)
            if (tid + j * NTHREADS < BW) {
                S.qblk[tid + j * NTHREADS] = qv[j];
                if (METRIC == COSINE) S.qq[tid + j * NTHREADS] = qv[j] * qv[j];
            }
        __syncthreads();
        VL_STAMP(5);
#pragma unroll
        for (int p = 0; p < NCH; ++p) {
            const uint32_t c0 = g0 + p * RP_CH;
            if (c0 >= dim) break;  // workgroup-uniform
            const uint32_t cw = (dim - c0) < (uint32_t)RP_CH ? (dim - c0) : (uint32_t)RP_CH;
            if (p) __syncthreads();  // the previous tile is consumed
#pragma unroll
            for (int i = 0; i < RP_PER; ++i) {
                const int idx = tid + i * NTHREADS;
                const int r = idx / RP_CH, cc = idx % RP_CH;
                const double x = pre[p][i], y = S.qblk[p * RP_CH + cc];
                if (METRIC == COSINE) {
                    S.tA[r][cc] = x * y;
                    S.tB[r][cc] = x * x;
                } else if (METRIC == EUCLIDEAN) {
                    const double d = x - y;
                    S.tA[r][cc] = d * d;
                } else if (METRIC == MANHATTAN) {
                    S.tA[r][cc] = fabs(x - y);
                } else {
                    S.tA[r][cc] = x * y;
                }
            }
            __syncthreads();
            if (wave == 0 || (METRIC == COSINE && wave == 1)) {
                if (lane < n_rows) {
                    const double* t = (wave == 0) ? &S.tA[lane][0] : &S.tB[METRIC == COSINE ? lane : 0][0];
                    uint32_t cc = 0;
                    for (; cc + 16 <= cw; cc += 16) {  // 16 LDS reads in flight, then 16 adds in index order
                        double v[16];
#pragma unroll
                        for (int u = 0; u < 16; ++u) v[u] = t[cc + u];
#pragma unroll
                        for (int u = 0; u < 16; ++u) acc += v[u];
                    }
                    for (; cc < cw; ++cc) acc += t[cc];
                }
            } else if (METRIC == COSINE && wave == 2) {
                // the query's own sum of squares, in index order like the rows': batched the same way -- one element per
                // LDS round trip made THIS wave the slowest of the three (0.84 -> 0.73 us per tile; the rest is barriers and the products)
                const double* t = &S.qq[p * RP_CH];
                uint32_t cc = 0;
                for (; cc + 16 <= cw; cc += 16) {
                    double v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) v[u] = t[cc + u];
#pragma unroll
                    for (int u = 0; u < 16; ++u) acc += v[u];
                }
                for (; cc < cw; ++cc) acc += t[cc];
            }
            if (p == 0) VL_STAMP(6);
        }
    }
    VL_STAMP(7);
    __syncthreads();
    if (METRIC == COSINE) {
        if (wave == 1 && lane < ROWS) S.b[lane] = acc;
        if (wave == 2 && lane == 0) S.c = acc;
        __syncthreads();
        if (wave == 0) {
            A.a = acc;
            A.b = S.b[lane < ROWS ? lane : 0];
            A.c = S.c;
        }
    } else if (wave == 0) {
        A.a = acc;
    }
}

// bound_for_key<METRIC> -- the upper bound on the reference score of any row whose scan key is <= t -- lives in
// score_bound.hpp: a range search evaluates the same function on the host.

// Phase 3 of a finalize, one WAVE per query: lane j holds candidate j's reference score and position (lanes >= n_cand hold
// nothing); key64 = the candidate list's 64th scan key.  Rank by (score desc, pos asc) = the reference's stable sort, run the
// exactness bound check, write the result block (and, for a row shard, its slice of the exchange record).
template <int METRIC>
__device__ __forceinline__ void rank_check_emit(double sc, uint32_t my_pos, float key64, int n_cand, uint32_t k, uint64_t n_rows,
                                                uint32_t ld, double R, double Q, double in_extra,
                                                SearchResultBlock* __restrict__ out, uint32_t seq, const ShardRecordSink& sink,
                                                uint32_t q_in_launch)
{
    const int lane = lane_id();
    const bool valid = lane < n_cand;
    const bool any_nan = __ballot(valid && sc != sc) != 0ull;
    // rank = how many candidates stand in front of this one: every candidate sits in a lane of this wave, so
    // entry j is read with v_readlane (a scalar operand of the compares), no LDS round trip per entry
    int rank = 0;
    for (int j = 0; j < n_cand; ++j) {
        const double sj = read_lane(sc, j);
        const uint32_t pj = read_lane(my_pos, j);
        rank += (sj > sc || (sj == sc && pj < my_pos)) ? 1 : 0;
    }
    const uint32_t k_eff = (uint64_t)k < n_rows ? k : (uint32_t)n_rows;
    uint32_t flags = 0;
    if (any_nan) flags |= RESULT_HAS_NAN | RESULT_NEEDS_EXACT;
    if (n_rows <= (uint64_t)KP) {
        // the list must hold EVERY row; a shorter one (a candidate stage that overflowed or dropped rows)
        // proves nothing
        if ((uint64_t)n_cand < n_rows) flags |= RESULT_NEEDS_EXACT;
    } else {
        // rows outside the candidate list exist: all of them have scan key <= the 64th key
        if (n_cand < KP) {
            flags |= RESULT_NEEDS_EXACT;  // keys were not finite: outside the fast-path domain
        } else {
            const double B = bound_for_key<METRIC>(key64, ld, R, Q, in_extra);
            // score of the entry ranked k_eff-1
            const unsigned long long at_cut = __ballot(valid && rank == (int)k_eff - 1);
            double s_cut = 0.0;
            if (at_cut) s_cut = __shfl(sc, __ffsll((long long)at_cut) - 1);
            if (!at_cut || !(s_cut > B)) flags |= RESULT_NEEDS_EXACT;
        }
    }
    if (valid && rank < (int)k_eff) {
        out->pos[rank] = my_pos;
        out->score[rank] = sc;
    }
    if (lane == 0) {
        out->n_out = k_eff;
        out->flags = flags;
    }
    if (sink.cnt) {  // a row shard's exchange record, written where the all-gather reads it (shard.hpp)
        const uint32_t q = sink.q0 + q_in_launch;
        const uint32_t offered = (flags == 0u) ? (k_eff < sink.ks ? k_eff : sink.ks) : 0u;  // not certified: the host redoes it
        if (valid && (uint32_t)rank < offered) {
            const size_t e = (size_t)q * sink.ks + (uint32_t)rank;
            sink.score_bits[e] = (unsigned long long)__double_as_longlong(sc);
            sink.gpos[e] = sink.row_offset + (unsigned long long)my_pos;
            sink.ids[e] = sink.pos_to_id[my_pos];
        }
        if (lane == 0) sink.cnt[q] = offered;
    }
    VL_STAMP(9);
    if (seq) {
        // the host spins on out->seq (pinned memory): every lane's stores of the block above are complete at
        // system scope before the stamp leaves (this wave is the only writer of the block)
        __threadfence_system();
        if (lane == 0) __hip_atomic_store(&out->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    VL_STAMP(10);
}

// A BATCH's finalize (n_lists = 1: the MFMA filter's one sorted top-64 list per query) as two launches.  k_merge_finalize
// spends a 1024-thread workgroup per query -- right for ONE search, where latency is everything -- but in a batch every
// workgroup then issues its 196 KB of row loads at once, waits for the memory system to serve all of them, and computes with
// one wave while 15 wait (1024 queries x 64 rows x 768 dimensions: 124 us = 3.2 TB/s of master rows).  Here a query's 64
// candidates are rescored by FOUR workgroups of 256 threads (16 rows each: 8 workgroups per CU, out of step with each other,
// so some load while others add), and a second launch of one wave per query ranks, checks the bound and emits.  Same
// arithmetic, same order: per row, products by all threads, one lane adds them in index order.
constexpr int BF_ROWS = 16;
#ifndef VL_BF_NCH
#define VL_BF_NCH 4
#endif
constexpr int BF_NCH = VL_BF_NCH;  // 48-column tiles fetched together: 4 = 192 columns in flight per thread (24 registers of row
                                   // data, 8 workgroups per CU); 8 = a dim-384 row in one round trip but 104 registers = 4 per CU
template <int METRIC>
__global__ __launch_bounds__(256) void k_batch_rescore(const Cand32* __restrict__ lists, const double* __restrict__ master,
                                                       const double* __restrict__ q64, uint32_t dim, double* __restrict__ scores)
{
    const uint32_t q = blockIdx.x >> 2, quarter = blockIdx.x & 3u;
    __shared__ RescoreLds<METRIC, BF_ROWS, BF_NCH> rs;
    __shared__ uint32_t sh_pos[BF_ROWS];
    __shared__ int sh_n;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const Cand32* mine = lists + (size_t)q * KP + quarter * BF_ROWS;
    q64 += (size_t)q * dim;
    constexpr int QN = (RP_CH * BF_NCH + 255) / 256;
    double q_first[QN];
#pragma unroll
    for (int j = 0; j < QN; ++j) {
        const uint32_t c = (uint32_t)(tid + j * 256);
        q_first[j] = q64[c < dim ? c : dim - 1];
    }
    if (wave == 0) {
        const uint32_t p = lane < BF_ROWS ? mine[lane].pos : POS_SENTINEL;
        if (lane < BF_ROWS) sh_pos[lane] = p;
        const unsigned long long real = __ballot(p != POS_SENTINEL);  // sorted list: the real entries come first
        if (lane == 0) sh_n = __popcll(real);
    }
    __syncthreads();
    const int n_mine = sh_n;
    Acc64<METRIC> A;
    rescore_rows_par<METRIC, BF_ROWS, 256, BF_NCH>(master, q64, dim, sh_pos, n_mine, rs, A, q_first);
    if (wave == 0 && lane < BF_ROWS) scores[(size_t)q * KP + quarter * BF_ROWS + lane] = lane < n_mine ? A.score() : 0.0;
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_batch_rank_emit(const Cand32* __restrict__ lists, const double* __restrict__ scores,
                                                         const double* __restrict__ q_norms, uint32_t nq, uint32_t ld,
                                                         uint64_t n_rows, uint32_t k, double R, double in_extra,
                                                         SearchResultBlock* __restrict__ out, ShardRecordSink sink)
{
    const int lane = lane_id();
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const Cand32 e = lists[(size_t)q * KP + lane];
    const int n_cand = __popcll(__ballot(e.pos != POS_SENTINEL));
    const double sc = lane < n_cand ? scores[(size_t)q * KP + lane] : 0.0;
    rank_check_emit<METRIC>(sc, e.pos, read_lane(e.key, KP - 1), n_cand, k, n_rows, ld, R, q_norms[q], in_extra, out + q, 0u, sink, q);
}

// k_batch_rank_emit for lists that hold only the rows each query's filter keeps (the masked MFMA filter, DESIGN.md section
// 24): the rows the bound check and the "a list of at most 64 rows must hold every row" rule refer to are the query's own
// m_of[q], and k is k_of[q] = min(k, m_of[q]) -- k_merge_finalize_jobs' arithmetic, read from two arrays.  Its own kernel,
// for the reason given there.
template <int METRIC>
__global__ __launch_bounds__(256) void k_batch_rank_emit_rows(const Cand32* __restrict__ lists, const double* __restrict__ scores,
                                                              const double* __restrict__ q_norms, uint32_t nq, uint32_t ld,
                                                              const uint32_t* __restrict__ m_of, const uint32_t* __restrict__ k_of,
                                                              double R, double in_extra, SearchResultBlock* __restrict__ out)
{
    const int lane = lane_id();
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const Cand32 e = lists[(size_t)q * KP + lane];
    const int n_cand = __popcll(__ballot(e.pos != POS_SENTINEL));
    const double sc = lane < n_cand ? scores[(size_t)q * KP + lane] : 0.0;
    rank_check_emit<METRIC>(sc, e.pos, read_lane(e.key, KP - 1), n_cand, k_of[q], (uint64_t)m_of[q], ld, R, q_norms[q], in_extra,
                            out + q, 0u, ShardRecordSink{}, q);
}

// The batched grouped search's stage behind k_batch_rescore: rank_check_emit's ranking and bound,
// then the collapse to one row per group, one WAVE per query, no LDS.  The lists hold rows of S only and n_rows = |S|.
// A candidate is CERTIFIED iff its score is > B = bound_for_key(the list's 64th key), strictly: no row outside the list
// scores above B, so it outranks all of them, and the certified candidates are a prefix of S's ranking.  (A list that
// holds all n_rows <= 64 rows has no row outside it: every candidate is certified.)  Inside the prefix a candidate is the
// first of its group iff no candidate of smaller rank has its group; its slot is the number of such candidates ranked
// before it.  Settled (flags == 0): k groups came out, or the whole of S was ranked and holds no NaN.
template <int METRIC>
__global__ __launch_bounds__(256) void k_batch_rank_collapse(const Cand32* __restrict__ lists, const double* __restrict__ scores,
                                                             const double* __restrict__ q_norms, uint32_t nq, uint32_t ld,
                                                             uint64_t n_rows, uint32_t k, double R, double in_extra,
                                                             const uint32_t* __restrict__ group_of_row, uint32_t index_rows,
                                                             GroupedResultBlock* __restrict__ out)
{
    const int lane = lane_id();
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const Cand32 e = lists[(size_t)q * KP + lane];
    const int n_cand = __popcll(__ballot(e.pos != POS_SENTINEL));
    const bool valid = lane < n_cand;
    const double sc = valid ? scores[(size_t)q * KP + lane] : 0.0;
    const uint32_t my_pos = e.pos;
    const bool any_nan = __ballot(valid && sc != sc) != 0ull;
    int rank = 0;  // (score desc, position asc), as rank_check_emit ranks
    for (int j = 0; j < n_cand; ++j) {
        const double sj = read_lane(sc, j);
        const uint32_t pj = read_lane(my_pos, j);
        rank += (sj > sc || (sj == sc && pj < my_pos)) ? 1 : 0;
    }
    uint32_t flags = 0;
    if (any_nan) flags |= RESULT_HAS_NAN | RESULT_NEEDS_EXACT;
    bool certified = false;
    bool complete = false;  // the list is the whole of S
    if (n_rows <= (uint64_t)KP) {
        complete = (uint64_t)n_cand >= n_rows;
        if (!complete) flags |= RESULT_NEEDS_EXACT;
        certified = valid && complete && !any_nan;
    } else if (n_cand < KP) {
        flags |= RESULT_NEEDS_EXACT;  // keys were not finite, or the candidate stage dropped rows
    } else {
        const double B = bound_for_key<METRIC>(read_lane(e.key, KP - 1), ld, R, q_norms[q], in_extra);
        certified = !any_nan && sc > B;
    }
    uint32_t g = GROUP_NONE;
    if (certified && my_pos < index_rows) g = group_of_row[my_pos];
    if (__ballot(certified && g == GROUP_NONE) != 0ull) {  // a row of S without a group: the bitmap and the table disagree
        flags |= RESULT_NEEDS_EXACT;
        certified = false;
    }
    uint32_t dup = 0;
    for (int j = 0; j < n_cand; ++j) {
        const uint32_t gj = read_lane(g, j);
        const uint32_t rj = read_lane((uint32_t)rank, j);
        dup |= (gj == g && rj < (uint32_t)rank) ? 1u : 0u;  // (an uncertified lane holds GROUP_NONE and is never `first`)
    }
    const uint32_t first = (certified && !dup) ? 1u : 0u;
    uint32_t slot = 0;
    for (int j = 0; j < n_cand; ++j) {
        const uint32_t fj = read_lane(first, j);
        const uint32_t rj = read_lane((uint32_t)rank, j);
        slot += (fj && rj < (uint32_t)rank) ? 1u : 0u;
    }
    const uint32_t n_first = (uint32_t)__popcll(__ballot(first != 0u));
    if (n_first < k && !(complete && !any_nan)) flags |= RESULT_NEEDS_EXACT;
    GroupedResultBlock* o = out + q;
    if (first && slot < k) {
        o->pos[slot] = my_pos;
        o->group[slot] = g;
        o->score[slot] = sc;
    }
    if (lane == 0) {  // the count and the flags last
        o->n_out = n_first < k ? n_first : k;
        o->flags = flags;
    }
}

// K2: merge partial lists, rescore, rank, bound-check.  One workgroup of 1024 threads.
template <int METRIC>
__global__ __launch_bounds__(1024) void k_merge_finalize(const Cand32* __restrict__ partials, int n_lists,
                                                         size_t list_stride_q, const double* __restrict__ master,
                                                         const double* __restrict__ q64,
                                                         const double* __restrict__ q_norms, uint32_t dim,
                                                         uint32_t ld, uint64_t n_rows, uint32_t k, double R,
                                                         double in_extra, SearchResultBlock* __restrict__ out,
                                                         uint32_t seq, ShardRecordSink sink)
{
    // one workgroup per query of the batch
    partials += (size_t)blockIdx.x * list_stride_q;
    q64 += (size_t)blockIdx.x * dim;
    out += blockIdx.x;
    const double Q = q_norms[blockIdx.x];
    constexpr int NW = 16;
    __shared__ Cand32 sh_lists[NW * WAVE];
    __shared__ RescoreLds<METRIC> rs;
    __shared__ uint32_t sh_pos[KP];
    __shared__ float sh_key[KP];
    __shared__ int sh_ncand;

    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;

    VL_STAMP(0);
    // phase 1: n_lists <= 64 sorted lists: up to 16 waves x 4 bitonic folds, then a tree merge over the waves that hold one
    TopList<float> L;
    double q_first[1] = {0.0};
    {
        const int first = wave * 4;
        int count = n_lists - first;
        count = count < 0 ? 0 : (count > 4 ? 4 : count);
        Cand32 e[4];
        fold_lists4_load<Cand32>(e, partials, first, count);
        // the query's first block is requested BEHIND the list loads (vector loads return in order: in front of
        // them the wave would sit out the pinned-memory round trip before it can merge) and is consumed only in phase 2
        if (threadIdx.x < RP_BW) q_first[0] = q64[threadIdx.x < dim ? threadIdx.x : dim - 1];
        fold_lists4_merge<float, Cand32>(L, e, count);
    }
    VL_STAMP(1);
    block_merge_n<float, Cand32>(L, sh_lists, (n_lists + 3) / 4);
    VL_STAMP(2);
    if (wave == 0) {
        sh_pos[lane] = L.pos;
        sh_key[lane] = L.key;
        const unsigned long long real = __ballot(L.pos != POS_SENTINEL);
        if (lane == 0) sh_ncand = __popcll(real);
    }
    __syncthreads();
    const int n_cand = sh_ncand;

    // phase 2: exact f64 rescoring of the candidates
    Acc64<METRIC> A;
    VL_STAMP(3);
    rescore_rows_par<METRIC, KP, 1024>(master, q64, dim, sh_pos, n_cand, rs, A, q_first);
    VL_STAMP(8);

    // phase 3: rank by (score desc, pos asc), bound check, emit
    if (wave == 0) {
        const bool valid = lane < n_cand;
        const double sc = valid ? A.score() : 0.0;
        rank_check_emit<METRIC>(sc, sh_pos[lane], sh_key[KP - 1], n_cand, k, n_rows, ld, R, Q, in_extra, out, seq, sink, blockIdx.x);
    }
}

// K2 per job of a filtered batch (k_scan_subset_jobs' lists): k_merge_finalize, phase by phase, except that the rows the
// bound check and the "a list of at most 64 rows must hold every row" rule refer to are the job's m and k is the job's
// min(k, m), both read from the job table.  Its own kernel, not a flag or a shared body of k_merge_finalize: folding the
// two changed the address arithmetic hipcc emits for k_merge_finalize's result block, and the kernels the unfiltered
// paths launch stay as they are.
template <int METRIC>
__global__ __launch_bounds__(1024) void k_merge_finalize_jobs(const Cand32* __restrict__ partials, int n_lists,
                                                              size_t list_stride_q, const double* __restrict__ master,
                                                              const double* __restrict__ q64,
                                                              const double* __restrict__ q_norms, uint32_t dim, uint32_t ld,
                                                              const SubsetJobDev* __restrict__ jobs, double R,
                                                              SearchResultBlock* __restrict__ out)
{
    // one workgroup per job of the launch
    partials += (size_t)blockIdx.x * list_stride_q;
    q64 += (size_t)blockIdx.x * dim;
    out += blockIdx.x;
    const double Q = q_norms[blockIdx.x];
    const SubsetJobDev job = jobs[blockIdx.x];
    constexpr int NW = 16;
    __shared__ Cand32 sh_lists[NW * WAVE];
    __shared__ RescoreLds<METRIC> rs;
    __shared__ uint32_t sh_pos[KP];
    __shared__ float sh_key[KP];
    __shared__ int sh_ncand;

    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;

    // phase 1: n_lists <= 64 sorted lists: up to 16 waves x 4 bitonic folds, then a tree merge over the waves that hold one
    TopList<float> L;
    double q_first[1] = {0.0};
    {
        const int first = wave * 4;
        int count = n_lists - first;
        count = count < 0 ? 0 : (count > 4 ? 4 : count);
        Cand32 e[4];
        fold_lists4_load<Cand32>(e, partials, first, count);
        if (threadIdx.x < RP_BW) q_first[0] = q64[threadIdx.x < dim ? threadIdx.x : dim - 1];  // behind the list loads
        fold_lists4_merge<float, Cand32>(L, e, count);
    }
    block_merge_n<float, Cand32>(L, sh_lists, (n_lists + 3) / 4);
    if (wave == 0) {
        sh_pos[lane] = L.pos;
        sh_key[lane] = L.key;
        const unsigned long long real = __ballot(L.pos != POS_SENTINEL);
        if (lane == 0) sh_ncand = __popcll(real);
    }
    __syncthreads();
    const int n_cand = sh_ncand;

    // phase 2: exact f64 rescoring of the candidates
    Acc64<METRIC> A;
    rescore_rows_par<METRIC, KP, 1024>(master, q64, dim, sh_pos, n_cand, rs, A, q_first);

    // phase 3: rank by (score desc, pos asc), bound check against the job's rows, emit
    if (wave == 0) {
        const bool valid = lane < n_cand;
        const double sc = valid ? A.score() : 0.0;
        rank_check_emit<METRIC>(sc, sh_pos[lane], sh_key[KP - 1], n_cand, job.k, (uint64_t)job.m, ld, R, Q, 0.0, out, 0u,
                                ShardRecordSink{}, blockIdx.x);
    }
}

// K2 for 60 < k <= 220: the workgroup lists are cut into P partitions (any partition of the rows will do), each
// keeps its own top 64, and all 64 P candidates are rescored and ranked together.  A row left out of partition
// p's list has scan key <= that list's 64th key t_p, so the answer stands iff score[k-1] > max_p B(t_p) -- the
// same proof as K2's, per partition.  On random data the 64th key of one of P partitions sits near global rank
// 64 P, so k up to ~ 64 P - 30 is certified; anything else falls back to the exact kernels as before.
constexpr int KMULTI_PARTS = 4;

template <int METRIC>
__global__ __launch_bounds__(1024) void k_merge_finalize_multi(const Cand32* __restrict__ lists, int n_lists,
                                                               size_t part_stride, int n_parts,
                                                               const double* __restrict__ master,
                                                               const double* __restrict__ q64,
                                                               const double* __restrict__ q_norms, uint32_t dim,
                                                               uint32_t ld, uint64_t n_rows, uint32_t k, double R,
                                                               SearchResultBlock* __restrict__ out)
{
    constexpr int NW = 16;
    __shared__ Cand32 sh_lists[NW * WAVE];
    __shared__ RescoreLds<METRIC> rs;
    __shared__ uint32_t sh_pos[KMULTI_PARTS * KP];
    __shared__ float sh_key[KMULTI_PARTS * KP];
    __shared__ double sh_score[KMULTI_PARTS * KP];
    __shared__ int sh_ncand[KMULTI_PARTS];
    __shared__ int sh_flags;
    __shared__ double sh_cut;
    __shared__ int sh_has_cut;
    const double Q = q_norms[0];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    double q_first[1] = {0.0};
    if (threadIdx.x < RP_BW) q_first[0] = q64[threadIdx.x < dim ? threadIdx.x : dim - 1];
    if (threadIdx.x == 0) {
        sh_flags = 0;
        sh_has_cut = 0;
        sh_cut = 0.0;
    }
    // phase 1: per partition, n_lists <= 64 sorted lists -> its top 64
    for (int p = 0; p < n_parts; ++p) {
        TopList<float> L;
        const int first = wave * 4;
        int count = n_lists - first;
        count = count < 0 ? 0 : (count > 4 ? 4 : count);
        fold_lists4<float, Cand32>(L, lists + (size_t)p * part_stride, first, count);
        block_merge<float, Cand32, NW>(L, sh_lists);
        if (wave == 0) {
            sh_pos[p * KP + lane] = L.pos;
            sh_key[p * KP + lane] = L.key;
            const unsigned long long real = __ballot(L.pos != POS_SENTINEL);
            if (lane == 0) sh_ncand[p] = __popcll(real);
        }
        __syncthreads();
    }
    // phase 2: exact f64 rescoring, 64 rows at a time through the same LDS tile
    for (int p = 0; p < n_parts; ++p) {
        Acc64<METRIC> A;
        rescore_rows_par<METRIC, KP, 1024>(master, q64, dim, sh_pos + p * KP, sh_ncand[p], rs, A, q_first);
        if (wave == 0) sh_score[p * KP + lane] = lane < sh_ncand[p] ? A.score() : 0.0;
        __syncthreads();
    }
    // phase 3: rank all candidates by (score desc, pos asc), bound check, emit
    const int t = threadIdx.x;
    const int total_slots = n_parts * KP;
    const bool valid = t < total_slots && (t % KP) < sh_ncand[t / KP];
    const double sc = valid ? sh_score[t] : 0.0;
    const uint32_t my_pos = t < total_slots ? sh_pos[t] : POS_SENTINEL;
    if (valid && sc != sc) atomicOr(&sh_flags, (int)(RESULT_HAS_NAN | RESULT_NEEDS_EXACT));
    int rank = 0;
    for (int j = 0; j < total_slots; ++j) {
        if ((j % KP) >= sh_ncand[j / KP]) continue;
        const double sj = sh_score[j];
        const uint32_t pj = sh_pos[j];
        rank += (sj > sc || (sj == sc && pj < my_pos)) ? 1 : 0;
    }
    const uint32_t k_eff = (uint64_t)k < n_rows ? k : (uint32_t)n_rows;
    if (valid && rank == (int)k_eff - 1) {
        sh_cut = sc;
        sh_has_cut = 1;
    }
    __syncthreads();
    if (valid && rank < (int)k_eff) {
        out[rank / KP].pos[rank % KP] = my_pos;
        out[rank / KP].score[rank % KP] = sc;
    }
    if (t == 0) {
        uint32_t flags = (uint32_t)sh_flags;
        int total = 0;
        double B = -1.0e300;
        bool excluded_rows = false;
        for (int p = 0; p < n_parts; ++p) {
            total += sh_ncand[p];
            if (sh_ncand[p] == KP) {  // a full list: rows behind its 64th key exist (or may exist)
                excluded_rows = true;
                const double bp = bound_for_key<METRIC>(sh_key[p * KP + KP - 1], ld, R, Q, 0.0);
                B = bp > B ? bp : B;
            }
        }
        if (!sh_has_cut || (uint32_t)total < k_eff) flags |= RESULT_NEEDS_EXACT;
        else if (excluded_rows && !(sh_cut > B)) flags |= RESULT_NEEDS_EXACT;
        if ((uint64_t)total < n_rows && !excluded_rows) flags |= RESULT_NEEDS_EXACT;  // short lists that do not cover the index
        out[0].n_out = k_eff;
        out[0].flags = flags;
    }
}

// ---------------------------------------------------------------------------------------------
// Exact path
// ---------------------------------------------------------------------------------------------
constexpr int EX_ROWS = 256;  // rows per workgroup tile (one per thread)
constexpr int EX_CH = 16;     // columns per chunk: 128 B of each row = one full line

template <int METRIC>
__global__ __launch_bounds__(256) void k_exact_scan(const double* __restrict__ master,
                                                    const double* __restrict__ q64, uint64_t n, uint32_t dim,
                                                    double* __restrict__ scores, uint32_t* __restrict__ nan_flag)
{
    // One thread owns one row and walks it in index order (the reference's serial f64 chains), so the rows
    // of a tile are transposed through LDS: 16 consecutive threads fetch one row's 128-byte line, then each
    // thread reads its own row from the padded tile.  The next chunk's loads are issued into registers
    // BEFORE the current chunk's arithmetic, so HBM latency hides behind the 16 dependent steps.
    __shared__ double tile[EX_ROWS][EX_CH + 1];
    __shared__ double qtile[EX_CH];
    const int tid = threadIdx.x;
    const uint64_t n_tiles = (n + EX_ROWS - 1) / EX_ROWS;
    const uint32_t n_chunks = (dim + EX_CH - 1) / EX_CH;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t row0 = t * EX_ROWS;
        const uint64_t rows_here = (n - row0) < (uint64_t)EX_ROWS ? (n - row0) : (uint64_t)EX_ROWS;
        Acc64<METRIC> A;
        A.init();
        double pre[EX_CH];
        double qpre = 0.0;
        auto fetch = [&](uint32_t c0) {
            const uint32_t cw = (dim - c0) < (uint32_t)EX_CH ? (dim - c0) : (uint32_t)EX_CH;
#pragma unroll
            for (int i = 0; i < EX_CH; ++i) {
                // clamped, never predicated: a load under a condition makes hipcc wait for each one in turn;
                // rows >= rows_here are never walked and columns >= cw never stepped, so duplicates are harmless
                const int idx = tid + i * 256;
                uint64_t r = (uint64_t)(idx / EX_CH);
                uint32_t cc = (uint32_t)(idx % EX_CH);
                r = r < rows_here ? r : rows_here - 1;
                cc = cc < cw ? cc : cw - 1;
                pre[i] = master[(row0 + r) * dim + c0 + cc];
            }
            {
                uint32_t qc = (uint32_t)(tid % EX_CH);
                qc = qc < cw ? qc : cw - 1;
                qpre = q64[c0 + qc];
            }
        };
        fetch(0);
        for (uint32_t ch = 0; ch < n_chunks; ++ch) {
            const uint32_t c0 = ch * EX_CH;
            const uint32_t cw = (dim - c0) < (uint32_t)EX_CH ? (dim - c0) : (uint32_t)EX_CH;
            __syncthreads();  // the previous chunk's readers are done with the tile
#pragma unroll
            for (int i = 0; i < EX_CH; ++i) {
                const int idx = tid + i * 256;
                tile[idx / EX_CH][idx % EX_CH] = pre[i];
            }
            if (tid < EX_CH) qtile[tid] = qpre;
            __syncthreads();
            if (ch + 1 < n_chunks) fetch(c0 + EX_CH);  // in flight during the arithmetic below
            if ((uint64_t)tid < rows_here) {
                if (cw == (uint32_t)EX_CH) {
#pragma unroll
                    for (uint32_t cc = 0; cc < (uint32_t)EX_CH; ++cc) A.step(tile[tid][cc], qtile[cc]);
                } else {
                    for (uint32_t cc = 0; cc < cw; ++cc) A.step(tile[tid][cc], qtile[cc]);
                }
            }
        }
        if ((uint64_t)tid < rows_here) {
            const double sc = A.score();
            scores[row0 + tid] = sc;
            if (sc != sc) atomicOr(nan_flag, 1u);
        }
    }
}

// k_exact_scan over a subset: scores[i] = the reference score of row plist[i], i < m.  The same tile walk and the same
// Acc64 steps (separate multiply and add, index order); only a tile row's source is plist[row0 + r] instead of row0 + r.
template <int METRIC>
__device__ __forceinline__ void exact_scan_subset_body(const double* __restrict__ master, const double* __restrict__ q64,
                                                       const uint32_t* __restrict__ plist, uint64_t m, uint32_t dim,
                                                       double* __restrict__ scores, uint32_t* __restrict__ nan_flag)
{
    __shared__ double tile[EX_ROWS][EX_CH + 1];
    __shared__ double qtile[EX_CH];
    const int tid = threadIdx.x;
    const uint64_t n_tiles = (m + EX_ROWS - 1) / EX_ROWS;
    const uint32_t n_chunks = (dim + EX_CH - 1) / EX_CH;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t row0 = t * EX_ROWS;
        const uint64_t rows_here = (m - row0) < (uint64_t)EX_ROWS ? (m - row0) : (uint64_t)EX_ROWS;
        // the storage rows this thread fetches from (the same for every chunk)
        uint64_t src[EX_CH];
#pragma unroll
        for (int i = 0; i < EX_CH; ++i) {
            uint64_t r = (uint64_t)((tid + i * 256) / EX_CH);
            r = r < rows_here ? r : rows_here - 1;
            src[i] = (uint64_t)plist[row0 + r] * dim;
        }
        Acc64<METRIC> A;
        A.init();
        double pre[EX_CH];
        double qpre = 0.0;
        auto fetch = [&](uint32_t c0) {
            const uint32_t cw = (dim - c0) < (uint32_t)EX_CH ? (dim - c0) : (uint32_t)EX_CH;
#pragma unroll
            for (int i = 0; i < EX_CH; ++i) {
                uint32_t cc = (uint32_t)((tid + i * 256) % EX_CH);
                cc = cc < cw ? cc : cw - 1;
                pre[i] = master[src[i] + c0 + cc];
            }
            {
                uint32_t qc = (uint32_t)(tid % EX_CH);
                qc = qc < cw ? qc : cw - 1;
                qpre = q64[c0 + qc];
            }
        };
        fetch(0);
        for (uint32_t ch = 0; ch < n_chunks; ++ch) {
            const uint32_t c0 = ch * EX_CH;
            const uint32_t cw = (dim - c0) < (uint32_t)EX_CH ? (dim - c0) : (uint32_t)EX_CH;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < EX_CH; ++i) {
                const int idx = tid + i * 256;
                tile[idx / EX_CH][idx % EX_CH] = pre[i];
            }
            if (tid < EX_CH) qtile[tid] = qpre;
            __syncthreads();
            if (ch + 1 < n_chunks) fetch(c0 + EX_CH);
            if ((uint64_t)tid < rows_here) {
                if (cw == (uint32_t)EX_CH) {
#pragma unroll
                    for (uint32_t cc = 0; cc < (uint32_t)EX_CH; ++cc) A.step(tile[tid][cc], qtile[cc]);
                } else {
                    for (uint32_t cc = 0; cc < cw; ++cc) A.step(tile[tid][cc], qtile[cc]);
                }
            }
        }
        if ((uint64_t)tid < rows_here) {
            const double sc = A.score();
            scores[row0 + tid] = sc;
            if (sc != sc) atomicOr(nan_flag, 1u);
        }
    }
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_exact_scan_subset(const double* __restrict__ master,
                                                           const double* __restrict__ q64,
                                                           const uint32_t* __restrict__ plist, uint64_t m, uint32_t dim,
                                                           double* __restrict__ scores, uint32_t* __restrict__ nan_flag)
{
    exact_scan_subset_body<METRIC>(master, q64, plist, m, dim, scores, nan_flag);
}

// Range search: the reference score of every candidate the range scan appended, scores[i] for cand[i], i < ctr[0] -- the
// count is read on the device, no host round trip stands between the scan and this kernel.  A counter above `cap` means
// the candidate buffer overflowed: nothing is done, the host takes the exact route.  ctr[2] is the NaN flag.
template <int METRIC>
__global__ __launch_bounds__(256) void k_range_rescore(const double* __restrict__ master, const double* __restrict__ q64,
                                                       const uint32_t* __restrict__ cand, uint32_t cap, uint32_t dim,
                                                       double* __restrict__ scores, uint32_t* __restrict__ ctr)
{
    const uint32_t m = ctr[RANGE_CTR_APPENDED];
    if (m == 0 || m > cap) return;
    exact_scan_subset_body<METRIC>(master, q64, cand, (uint64_t)m, dim, scores, ctr + RANGE_CTR_NAN);
}

// top-64 of scores[] by (score desc, pos asc): per-wave lists, then per-workgroup merge
// `after` (optional): the result block of the previous round; only rows ranked strictly behind its last
// entry are offered, so round r yields ranks 64 r .. 64 r + 63 of the full (score desc, pos asc) order.
__global__ __launch_bounds__(256) void k_select64(const double* __restrict__ scores, uint32_t n,
                                                  const SearchResultBlock* __restrict__ after,
                                                  Cand64* __restrict__ out)
{
    __shared__ Cand64 sh[4 * WAVE];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const uint32_t n_steps = (n + WAVE - 1) / WAVE;
    const uint32_t n_waves = gridDim.x * 4;
    TopList<double> L;
    L.init();
    const bool cut = after != nullptr;
    const double cut_key = cut ? after->score[KP - 1] : 0.0;
    const uint32_t cut_pos = cut ? after->pos[KP - 1] : 0u;
    for (uint32_t s = blockIdx.x * 4 + wave; s < n_steps; s += n_waves) {
        const uint32_t row = s * WAVE + lane;
        bool valid = row < n;
        const double sc = valid ? scores[row] : 0.0;
        if (cut) valid = valid && better<double>(cut_key, cut_pos, sc, row);
        L.offer(sc, row, valid);
    }
    block_merge<double, Cand64, 4>(L, sh);
    if (wave == 0) {
        Cand64 e;
        e.key = L.key;
        e.pos = L.pos;
        e.pad = 0;
        out[(size_t)blockIdx.x * KP + lane] = e;
    }
}

__global__ __launch_bounds__(1024) void k_merge64_emit(const Cand64* __restrict__ partials, int n_lists,
                                                       uint64_t n_rows, uint32_t k,
                                                       const uint32_t* __restrict__ nan_flag,
                                                       SearchResultBlock* __restrict__ out)
{
    constexpr int NW = 16;
    __shared__ Cand64 sh[NW * WAVE];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    TopList<double> L;
    {
        const int first = wave * 4;
        int count = n_lists - first;
        count = count < 0 ? 0 : (count > 4 ? 4 : count);
        fold_lists4<double, Cand64>(L, partials, first, count);
    }
    block_merge<double, Cand64, NW>(L, sh);
    if (wave == 0) {
        const uint32_t k_eff = (uint64_t)k < n_rows ? k : (uint32_t)n_rows;
        if ((uint32_t)lane < k_eff || k == (uint32_t)KP) {  // a full round also carries its cut entry for the next one
            out->pos[lane] = L.pos;
            out->score[lane] = L.key;
        }
        if (lane == 0) {
            out->n_out = k_eff;
            out->flags = (*nan_flag) ? RESULT_HAS_NAN : 0u;
        }
    }
}

// ---- device-wide bitonic sort on (score desc, pos asc) for k > 64 ------------------------------
// okey: u64 whose ASCENDING unsigned order is the DESCENDING order of the score (-0.0 == +0.0).
__device__ __forceinline__ unsigned long long desc_key(double s)
{
    s = s + 0.0;  // -0.0 -> +0.0: partial_cmp treats them as equal
    unsigned long long b = (unsigned long long)__double_as_longlong(s);
    const unsigned long long asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return ~asc;
}

__global__ void k_sort_init(const double* __restrict__ scores, uint64_t n, uint64_t cap,
                            unsigned long long* __restrict__ okeys, uint32_t* __restrict__ opos)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < cap;
         i += (uint64_t)gridDim.x * blockDim.x) {
        if (i < n) {
            okeys[i] = desc_key(scores[i]);
            opos[i] = (uint32_t)i;
        } else {
            okeys[i] = ~0ull;
            opos[i] = POS_SENTINEL;
        }
    }
}

// P: the payload that breaks ties -- a u32 position (the exact sort: index = position), or a range search's u64
// (position << 32 | slot of the score)
template <typename P>
__device__ __forceinline__ bool pair_greater(unsigned long long ka, P pa, unsigned long long kb, P pb)
{
    return ka > kb || (ka == kb && pa > pb);
}

constexpr int SORT_LOCAL = 2048;  // elements sorted in LDS by one 1024-thread workgroup
static_assert((uint32_t)SORT_LOCAL == RANGE_SMALL, "a range search's speculative ranking is one local sort");

// All stages with j < SORT_LOCAL for k in [k_lo, k_hi] (k_lo == k_hi > SORT_LOCAL: tail of one k).
template <typename P>
__global__ __launch_bounds__(1024) void k_bitonic_local(unsigned long long* __restrict__ okeys, P* __restrict__ opos,
                                                        uint64_t k_lo, uint64_t k_hi)
{
    __shared__ unsigned long long sk[SORT_LOCAL];
    __shared__ P sp[SORT_LOCAL];
    const uint64_t base = (uint64_t)blockIdx.x * SORT_LOCAL;
    const int tid = threadIdx.x;
    sk[tid] = okeys[base + tid];
    sp[tid] = opos[base + tid];
    sk[tid + 1024] = okeys[base + tid + 1024];
    sp[tid + 1024] = opos[base + tid + 1024];
    __syncthreads();
    for (uint64_t k = k_lo; k <= k_hi; k <<= 1) {
        uint64_t j = (k >> 1) < (uint64_t)(SORT_LOCAL >> 1) ? (k >> 1) : (uint64_t)(SORT_LOCAL >> 1);
        for (; j >= 1; j >>= 1) {
            // thread t handles the pair (i, i ^ j) with i the t-th index whose bit j is clear
            const uint32_t jj = (uint32_t)j;
            const uint32_t i = ((tid & ~(jj - 1)) << 1) | (tid & (jj - 1));
            const uint32_t l = i | jj;
            const bool up = (((base + i) & k) == 0);
            const unsigned long long ka = sk[i], kb = sk[l];
            const P pa = sp[i], pb = sp[l];
            const bool gt = pair_greater<P>(ka, pa, kb, pb);
            if (gt == up) {
                sk[i] = kb;
                sp[i] = pb;
                sk[l] = ka;
                sp[l] = pa;
            }
            __syncthreads();
        }
    }
    okeys[base + tid] = sk[tid];
    opos[base + tid] = sp[tid];
    okeys[base + tid + 1024] = sk[tid + 1024];
    opos[base + tid + 1024] = sp[tid + 1024];
}

template <typename P>
__global__ void k_bitonic_global(unsigned long long* __restrict__ okeys, P* __restrict__ opos, uint64_t cap, uint64_t j,
                                 uint64_t k)
{
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < (cap >> 1);
         t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint64_t l = i | j;
        const bool up = ((i & k) == 0);
        const unsigned long long ka = okeys[i], kb = okeys[l];
        const P pa = opos[i], pb = opos[l];
        if (pair_greater<P>(ka, pa, kb, pb) == up) {
            okeys[i] = kb;
            opos[i] = pb;
            okeys[l] = ka;
            opos[l] = pa;
        }
    }
}

__global__ void k_sort_emit(const uint32_t* __restrict__ opos, const double* __restrict__ scores, uint64_t k,
                            uint32_t* __restrict__ out_pos, double* __restrict__ out_scores)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < k;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = opos[i];
        out_pos[i] = p;
        out_scores[i] = scores[p];
    }
}

// ---- range search: cut at the threshold, rank, emit ---------------------------------------------
// The cut: every slot i < m whose score satisfies the IEEE comparison score >= min_score is appended (one atomic per wave)
// to (keys, pv) as (desc_key(score), position << 32 | i); ctr[RANGE_CTR_TOTAL] counts them all, entries past
// `store_cap` are counted and not stored (store_cap = 0: count only).  cand == nullptr: slot i IS the position (the exact
// route's scores[] of every row); else the position is cand[i] (the fast route's candidates, or a filter's list).
// m_ptr != nullptr: m is the range scan's counter, and nothing is done when it ran past cap_in.
template <bool GROUPED>
__global__ __launch_bounds__(256) void k_range_cut(const double* __restrict__ scores, const uint32_t* __restrict__ cand,
                                                   const uint32_t* __restrict__ m_ptr, uint32_t m_val, uint32_t cap_in,
                                                   double min_score, unsigned long long* __restrict__ keys,
                                                   unsigned long long* __restrict__ pv, uint32_t store_cap,
                                                   uint32_t* __restrict__ ctr, const uint32_t* __restrict__ group_of_row,
                                                   uint32_t n_rows, int keep_nan)
{
    const uint32_t m = m_ptr ? *m_ptr : m_val;
    if (m_ptr && m > cap_in) return;
    const int lane = lane_id();
    const uint32_t step = gridDim.x * 256;
    for (uint32_t b0 = blockIdx.x * 256; b0 < m; b0 += step) {  // workgroup-uniform trip count
        const uint32_t i = b0 + threadIdx.x;
        const bool valid = i < m;
        const double sc = scores[valid ? i : m - 1];
        bool keep = valid && sc >= min_score;
        if constexpr (GROUPED) {
            // a grouped search's cut: rows without a group take no part; keep_nan (its exact route): NaN scores stay in and
            // are counted, so that the host knows |S| and whether the reference's sort would have met a NaN
            const uint32_t pos = cand ? cand[valid ? i : m - 1] : i;
            const bool grouped = valid && pos < n_rows && group_of_row[pos] != GROUP_NONE;
            const bool is_nan = sc != sc;
            if (grouped && is_nan && keep_nan) atomicAdd(ctr + RANGE_CTR_GROUP_NAN, 1u);
            keep = grouped && (keep || (is_nan && keep_nan));
        }
        const unsigned long long bal = __ballot(keep);
        if (bal == 0ull) continue;  // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(ctr + RANGE_CTR_TOTAL, (uint32_t)__popcll(bal));
        base = __shfl(base, 0);
        const uint32_t slot = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (keep && slot < store_cap) {
            const uint32_t pos = cand ? cand[i] : i;
            keys[slot] = desc_key(sc);
            pv[slot] = ((unsigned long long)pos << 32) | (unsigned long long)i;
        }
    }
}

// Pads (keys, pv) from the survivor count up to the sort's capacity with entries that sort last.  total_ptr != nullptr:
// the count is ctr's (the speculative small sort, before the host knows it); a count above `cap` leaves the buffers alone.
__global__ void k_range_pad(unsigned long long* __restrict__ keys, unsigned long long* __restrict__ pv,
                            const uint32_t* __restrict__ total_ptr, uint64_t total_val, uint64_t cap)
{
    const uint64_t total = total_ptr ? (uint64_t)*total_ptr : total_val;
    if (total > cap) return;
    for (uint64_t i = total + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
        keys[i] = ~0ull;
        pv[i] = ~0ull;
    }
}

// The first min(total, k) entries of the sorted (keys, pv): position and the score's own bits (scores[slot]).
__global__ void k_range_emit(const unsigned long long* __restrict__ pv, const double* __restrict__ scores,
                             const uint32_t* __restrict__ total_ptr, uint64_t k, uint32_t* __restrict__ out_pos,
                             double* __restrict__ out_scores)
{
    if (total_ptr && (uint64_t)*total_ptr < k) k = *total_ptr;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < k; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long e = pv[i];
        out_pos[i] = (uint32_t)(e >> 32);
        out_scores[i] = scores[(uint32_t)e];
    }
}

// ---- batched range search: the segmented tail behind the MFMA filter's one pass ----------------
// Query q's candidates are cand[q * cap + i], i < cnt[q] (the filter's per-query buffers; a counter above cap means the
// buffer or a ring segment overflowed: the query is left alone and the host redoes it).  ctr: RBATCH_CTR_WORDS words per
// query, zeroed by the caller in front of each launch sequence.
//
// Rescore + cut: workgroup (x, q) rescores tiles x, x + gridDim.x, ... of 16 candidates of query q with the batch
// finalize's rescore_rows_par (products by all threads, one lane per row adds them in index order: the reference's
// arithmetic, many rows and queries in flight), then cuts on score >= min_scores[q]: survivors are appended (one atomic per
// tile) as (score, position) to the query's segment of RBATCH_SEG entries; ctr[TOTAL] counts them all.
template <int METRIC>
__global__ __launch_bounds__(256) void k_rbatch_rescore_cut(const Cand32* __restrict__ cand, const uint32_t* __restrict__ cnt,
                                                            uint32_t cap, const double* __restrict__ master,
                                                            const double* __restrict__ q64, const double* __restrict__ min_scores,
                                                            uint32_t dim, uint32_t n_rows, double* __restrict__ sv_score,
                                                            uint32_t* __restrict__ sv_pos, uint32_t* __restrict__ ctr)
{
    const uint32_t q = blockIdx.y;
    const uint32_t m = cnt[q];
    if (m == 0 || m > cap) return;  // workgroup-uniform
    __shared__ RescoreLds<METRIC, BF_ROWS, BF_NCH> rs;
    __shared__ uint32_t sh_pos[BF_ROWS];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const Cand32* mine = cand + (size_t)q * cap;
    q64 += (size_t)q * dim;
    const double cut = min_scores[q];
    uint32_t* my_ctr = ctr + (size_t)q * RBATCH_CTR_WORDS;
    constexpr int QN = (RP_CH * BF_NCH + 255) / 256;
    double q_first[QN];
#pragma unroll
    for (int j = 0; j < QN; ++j) {
        const uint32_t c = (uint32_t)(tid + j * 256);
        q_first[j] = q64[c < dim ? c : dim - 1];
    }
    for (uint32_t t0 = blockIdx.x * BF_ROWS; t0 < m; t0 += gridDim.x * BF_ROWS) {  // workgroup-uniform trip count
        const int n_here = (int)((m - t0) < (uint32_t)BF_ROWS ? (m - t0) : (uint32_t)BF_ROWS);
        __syncthreads();  // the previous tile's positions are consumed
        if (tid < BF_ROWS) {
            const uint32_t p = mine[t0 + (uint32_t)(tid < n_here ? tid : n_here - 1)].pos;
            sh_pos[tid] = p < n_rows ? p : n_rows - 1;
        }
        __syncthreads();
        Acc64<METRIC> A;
        rescore_rows_par<METRIC, BF_ROWS, 256, BF_NCH>(master, q64, dim, sh_pos, n_here, rs, A, q_first);
        if (wave == 0) {
            const bool valid = lane < n_here;
            const double sc = valid ? A.score() : 0.0;
            if (valid && sc != sc) atomicOr(my_ctr + RBATCH_CTR_NAN, 1u);
            const bool keep = valid && sc >= cut;
            const unsigned long long bal = __ballot(keep);
            if (bal != 0ull) {  // wave-uniform
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(my_ctr + RBATCH_CTR_TOTAL, (uint32_t)__popcll(bal));
                base = __shfl(base, 0);
                const uint32_t slot = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                if (keep && slot < RBATCH_SEG) {
                    sv_score[(size_t)q * RBATCH_SEG + slot] = sc;
                    sv_pos[(size_t)q * RBATCH_SEG + slot] = sh_pos[lane];
                }
            }
        }
    }
}

// Where each query's answer goes in the packed output: want[q] = min(total, emit_cap) for a query the device answers
// (candidate buffer not overflowed, no NaN score, at most RBATCH_SEG survivors), 0 otherwise; off[q] = the sum of the
// want[] in front of it.  One workgroup.
__global__ __launch_bounds__(256) void k_rbatch_offsets(const uint32_t* __restrict__ cnt, uint32_t cap, uint32_t nq, uint32_t emit_cap,
                                                        uint32_t* __restrict__ ctr)
{
    __shared__ uint32_t part[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (nq + 255u) / 256u;
    const uint32_t q0 = tid * per, q1 = (q0 + per) < nq ? (q0 + per) : nq;
    uint32_t sum = 0;
    for (uint32_t q = q0; q < q1; ++q) {
        uint32_t* c = ctr + (size_t)q * RBATCH_CTR_WORDS;
        const uint32_t total = c[RBATCH_CTR_TOTAL];
        const bool ok = cnt[q] <= cap && c[RBATCH_CTR_NAN] == 0u && total <= RBATCH_SEG;
        const uint32_t want = ok ? (total < emit_cap ? total : emit_cap) : 0u;
        c[RBATCH_CTR_WANT] = want;
        sum += want;
    }
    part[tid] = sum;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t i = 0; i < tid; ++i) off += part[i];
    for (uint32_t q = q0; q < q1; ++q) {
        uint32_t* c = ctr + (size_t)q * RBATCH_CTR_WORDS;
        c[RBATCH_CTR_OFF] = off;
        off += c[RBATCH_CTR_WANT];
    }
}

// Segmented rank + emit, one workgroup per query: the survivors go to LDS as (desc_key(score), position << 32 | slot),
// padded to a power of two with entries that sort last; k_bitonic_local's network on pair_greater orders them by (score
// desc with -0.0 == +0.0, position asc); the first want[q] leave as (position, the score's own bits) at off[q].
__global__ __launch_bounds__(256) void k_rbatch_rank_emit(const double* __restrict__ sv_score, const uint32_t* __restrict__ sv_pos,
                                                          const uint32_t* __restrict__ ctr, uint32_t* __restrict__ out_pos,
                                                          double* __restrict__ out_scores)
{
    __shared__ unsigned long long sk[RBATCH_SEG];
    __shared__ unsigned long long sp[RBATCH_SEG];
    const uint32_t q = blockIdx.x;
    const uint32_t* c = ctr + (size_t)q * RBATCH_CTR_WORDS;
    const uint32_t want = c[RBATCH_CTR_WANT];
    if (want == 0) return;  // workgroup-uniform: nothing to emit, or the host redoes this query
    const uint32_t total = c[RBATCH_CTR_TOTAL], off = c[RBATCH_CTR_OFF];  // total <= RBATCH_SEG (k_rbatch_offsets)
    uint32_t n2 = 2;
    while (n2 < total) n2 <<= 1;
    const uint32_t tid = threadIdx.x;
    const double* my_score = sv_score + (size_t)q * RBATCH_SEG;
    const uint32_t* my_pos = sv_pos + (size_t)q * RBATCH_SEG;
    for (uint32_t i = tid; i < n2; i += 256) {
        const bool real = i < total;
        sk[i] = real ? desc_key(my_score[i]) : ~0ull;
        sp[i] = real ? (((unsigned long long)my_pos[i] << 32) | (unsigned long long)i) : ~0ull;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        for (uint32_t j = k >> 1; j >= 1; j >>= 1) {
            for (uint32_t t = tid; t < (n2 >> 1); t += 256) {  // pair (i, i ^ j), i the t-th index whose bit j is clear
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint32_t l = i | j;
                const bool up = ((i & k) == 0);
                const unsigned long long ka = sk[i], kb = sk[l];
                const unsigned long long pa = sp[i], pb = sp[l];
                if (pair_greater<unsigned long long>(ka, pa, kb, pb) == up) {
                    sk[i] = kb;
                    sp[i] = pb;
                    sk[l] = ka;
                    sp[l] = pa;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < want; i += 256) {
        const unsigned long long e = sp[i];
        out_pos[off + i] = (uint32_t)(e >> 32);
        out_scores[off + i] = my_score[(uint32_t)e];
    }
}

// ---------------------------------------------------------------------------------------------
// HNSW distance callbacks
// ---------------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256) void k_hnsw_dist(const double* __restrict__ master,
                                                   const double* __restrict__ q64, uint32_t dim,
                                                   const uint32_t* __restrict__ positions, uint32_t m,
                                                   unsigned long long* __restrict__ out)
{
    __shared__ double tile[KP][RESCORE_CH + 1];
    __shared__ double qtile[RESCORE_CH];
    __shared__ uint32_t sh_pos[KP];
    const uint32_t base = blockIdx.x * KP;
    const int n_here = (m - base) < (uint32_t)KP ? (int)(m - base) : KP;
    if (threadIdx.x < (unsigned)n_here) sh_pos[threadIdx.x] = positions[base + threadIdx.x];
    __syncthreads();
    Acc64<METRIC> A;
    // the reference calls distance(query, stored) (a = query); every callback is symmetric in
    // (a, b) bit for bit: x*y and |x-y| commute, (x-y)^2 == (y-x)^2.
    rescore_rows<METRIC, 256>(master, q64, dim, sh_pos, n_here, tile, qtile, A);
    if (threadIdx.x < (unsigned)n_here) out[base + threadIdx.x] = hnsw_quantise<METRIC>(A);
}

// ---------------------------------------------------------------------------------------------
// Ingest: f64 master rows -> f32 slab + 1/|row| cache + domain flags
// ---------------------------------------------------------------------------------------------
// One row, one wave: `src` is the row's f64 values (the master row itself, or an update's staged copy of it), `row` the
// position whose slab row, inv_norm and flag it writes.  Lane 0 returns the flag it stored.
__device__ __forceinline__ uint8_t ingest_row(const double* __restrict__ src, uint64_t row, float* __restrict__ slab,
                                              float* __restrict__ inv_norm, uint8_t* __restrict__ flags,
                                              IngestStats* __restrict__ stats, uint32_t dim, uint32_t ld, int lane)
{
    float* dst = slab + row * ld;
    double ss = 0.0, mx = 0.0;
    bool bad = false;
    for (uint32_t c = lane; c < ld; c += WAVE) {
        const double v = c < dim ? src[c] : 0.0;
        dst[c] = (float)v;  // round to nearest even
        ss += v * v;
        const double av = fabs(v);
        mx = av > mx ? av : mx;
        bad |= !(av <= 1.797693134862315708e308);  // inf or NaN
    }
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) {
        ss += __shfl_xor(ss, o);
        const double m2 = __shfl_xor(mx, o);
        mx = m2 > mx ? m2 : mx;
    }
    const bool any_bad = __ballot(bad) != 0ull;
    uint8_t flag = 0;
    if (lane == 0) {
        const double norm = sqrt(ss);
        const bool ood = any_bad || !(mx <= 1099511627776.0 /* 2^40 */) || !(norm <= 1.0e300) ||
                         (norm != 0.0 && norm < 9.094947017729282e-13 /* 2^-40 */);
        inv_norm[row] = (norm > 0.0 && !ood) ? (float)(1.0 / norm) : 0.0f;
        flag = ood ? ROW_OUT_OF_DOMAIN : 0;
        flags[row] = flag;
        if (ood) {
            atomicAdd(&stats->n_out_of_domain, 1u);
        } else {
            atomicMax(&stats->max_norm_bits, (unsigned long long)__double_as_longlong(norm));
        }
    }
    return flag;
}

__global__ __launch_bounds__(256) void k_ingest(const double* __restrict__ master, float* __restrict__ slab,
                                                float* __restrict__ inv_norm, uint8_t* __restrict__ flags,
                                                IngestStats* __restrict__ stats, uint64_t n, uint32_t dim,
                                                uint32_t ld)
{
    const int lane = lane_id();
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += n_waves)
        (void)ingest_row(master + row * dim, row, slab, inv_norm, flags, stats, dim, ld, lane);
}

// In-place update (GpuFlatIndex::update_bulk): staged row i (f64, [m, dim]) replaces the row at
// position pos[i] -- its master row, copied in 16-byte pieces where V == 16 (dim even: every row of both arrays starts on
// a 16-byte boundary), and what k_ingest derives from it, by k_ingest's own row body (same lanes, same order of sums: the
// bits a from-scratch ingest of the new master would write).  out_flags[i] = the row's new flag, for the host's
// bookkeeping.  Positions are distinct: no two waves write one row.  One wave per row.
template <int V>
__global__ __launch_bounds__(256) void k_update_rows(const double* __restrict__ staged, const uint32_t* __restrict__ pos,
                                                     uint32_t m, double* __restrict__ master, float* __restrict__ slab,
                                                     float* __restrict__ inv_norm, uint8_t* __restrict__ flags,
                                                     uint8_t* __restrict__ out_flags, IngestStats* __restrict__ stats,
                                                     uint32_t dim, uint32_t ld)
{
    const int lane = lane_id();
    const uint32_t n_waves = gridDim.x * 4;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += n_waves) {
        const double* src = staged + (uint64_t)i * dim;
        const uint64_t row = pos[i];
        double* mrow = master + row * dim;
        if (V == 16) {
            const double2* s2 = reinterpret_cast<const double2*>(src);
            double2* m2 = reinterpret_cast<double2*>(mrow);
            for (uint32_t c = lane; c < dim / 2; c += WAVE) m2[c] = s2[c];
        } else {
            for (uint32_t c = lane; c < dim; c += WAVE) mrow[c] = src[c];
        }
        const uint8_t flag = ingest_row(src, row, slab, inv_norm, flags, stats, dim, ld, lane);
        if (lane == 0) out_flags[i] = flag;
    }
}

// ---------------------------------------------------------------------------------------------
// Embedding ingest: the model's f32 output -> the f64 row the index stores, with the
// arithmetic of src/embeddings.rs:171-179: x as f64; norm = sqrt(sum of x*x in index order);
// x / norm when norm > 0, the widened values unchanged otherwise.
// One wave owns 64 rows per trip: the rows' columns go through a padded LDS tile 64 at a time (coalesced
// 256-byte reads), lane r then adds row r's squares in index order; the scaled rows are written
// coalesced, each lane fetching its row's norm by shuffle.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_embed_f32(const float* __restrict__ emb, uint64_t n, uint32_t dim,
                                                   int normalize, double* __restrict__ out)
{
    __shared__ float tile[4][WAVE][WAVE + 1];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t n_groups = (n + WAVE - 1) / WAVE;
    // every wave of a workgroup runs the same trips (the barriers below), rows past n are skipped
    for (uint64_t g0 = (uint64_t)blockIdx.x * 4; g0 < n_groups; g0 += (uint64_t)gridDim.x * 4) {
        const uint64_t base = (g0 + wave) * WAVE;
        double ss = -0.0;  // `.sum::<f64>()` folds from -0.0
        if (normalize) {
            for (uint32_t c0 = 0; c0 < dim; c0 += WAVE) {
                const uint32_t c = c0 + lane;
                __syncthreads();
                for (int rr = 0; rr < WAVE; ++rr) {
                    const uint64_t row = base + rr;
                    tile[wave][rr][lane] = (row < n && c < dim) ? emb[row * dim + c] : 0.f;
                }
                __syncthreads();
                const uint32_t w = dim - c0 < (uint32_t)WAVE ? dim - c0 : (uint32_t)WAVE;
                for (uint32_t j = 0; j < w; ++j) {
                    const double v = (double)tile[wave][lane][j];
                    ss += v * v;
                }
            }
        }
        const double norm = sqrt(ss);
        const int scale = (normalize && norm > 0.0) ? 1 : 0;
        for (int rr = 0; rr < WAVE; ++rr) {
            const uint64_t row = base + rr;
            if (row >= n) break;  // wave-uniform
            const double nr = __shfl(norm, rr);
            const int sc = __shfl(scale, rr);
            for (uint32_t c = lane; c < dim; c += WAVE) {
                const double v = (double)emb[row * dim + c];
                out[row * dim + c] = sc ? v / nr : v;
            }
        }
    }
}

// The same arithmetic for a FEW rows (a batch of query embeddings): one wave per row instead of one lane per row, so
// that 1024 rows fill the chip (k_embed_f32 keeps 16 waves busy on them: 484 us at dim 768).  The lanes square the row's
// values in parallel into LDS; ONE lane adds them in index order (the reference's `.sum::<f64>()` is sequential, and so
// is this chain: dim dependent f64 adds); the scaled row is written coalesced.  Rows of at most EMBED_ROW_MAX values.
constexpr uint32_t EMBED_ROW_MAX = 2048;

__global__ __launch_bounds__(256) void k_embed_f32_rows(const float* __restrict__ emb, uint64_t n, uint32_t dim,
                                                        int normalize, double* __restrict__ out)
{
    __shared__ double sq[4][EMBED_ROW_MAX];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + wave;
    if (row >= n) return;  // wave-uniform; no workgroup barrier below
    const float* x = emb + row * dim;
    double ss = -0.0;  // `.sum::<f64>()` folds from -0.0
    if (normalize) {
        for (uint32_t c = lane; c < dim; c += WAVE) {
            const double v = (double)x[c];
            sq[wave][c] = v * v;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's LDS writes have landed
        if (lane == 0) {
            uint32_t c = 0;
            for (; c + 8 <= dim; c += 8) {  // 8 LDS reads in flight, then 8 adds in index order
                double t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = sq[wave][c + j];
#pragma unroll
                for (int j = 0; j < 8; ++j) ss += t[j];
            }
            for (; c < dim; ++c) ss += sq[wave][c];
        }
        ss = __shfl(ss, 0);
    }
    const double norm = sqrt(ss);
    const bool scale = normalize && norm > 0.0;
    for (uint32_t c = lane; c < dim; c += WAVE) {
        const double v = (double)x[c];
        out[row * dim + c] = scale ? v / norm : v;
    }
}

// ---------------------------------------------------------------------------------------------
// Bulk delete (delete_plan.hpp): one launch moves the kept rows of one segment of destination rows up to their place in
// one device array, or gathers them into the bounce buffer.  A pure copy in units of V bytes (16 where the row pitch
// allows, 8 for f64 rows of odd dimension, 4 and 1 for the two per-row arrays): nothing is converted, a slab row's
// padding columns travel with it.
// Destination row d reads source row d + shift(d), shift(d) = #{i : keys[i] <= d} with keys[i] = r_i - i over the
// ascending removed positions; the segment's shifts lie in [c_lo, c_hi], so only keys[c_lo, c_hi) is searched.  A wave
// takes MOVE_U groups of rows per trip (a group = the rows 64 lanes cover at lpr lanes per row) and first searches for
// the trip's first and last row with wave-uniform (scalar) loads: holes are rare against rows, the two shifts are mostly
// equal and are then every lane's; otherwise each lane searches the few keys between them.  All loads of a trip's
// column step are issued before its stores (MOVE_U in flight per lane).
// src_base and dst may be the same array (a direct segment): the plan guarantees that the launch's destinations end
// before its sources begin, so no __restrict__ on them and nothing else is needed.
// ---------------------------------------------------------------------------------------------
constexpr int MOVE_U = 4;

template <int V> struct MoveUnit;
template <> struct MoveUnit<16> { typedef uint32_t type __attribute__((ext_vector_type(4))); };
template <> struct MoveUnit<8> { typedef uint32_t type __attribute__((ext_vector_type(2))); };
template <> struct MoveUnit<4> { using type = uint32_t; };
template <> struct MoveUnit<1> { using type = uint8_t; };

// lo + #{i in [lo, hi) : keys[i] <= d}
__device__ __forceinline__ uint32_t move_shift(const uint32_t* __restrict__ keys, uint32_t lo, uint32_t hi, uint32_t d)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] <= d) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int V>
__global__ __launch_bounds__(256) void k_move_rows(const char* src_base, char* dst, const uint32_t* __restrict__ keys,
                                                   uint32_t c_lo, uint32_t c_hi, uint32_t dst_begin, uint32_t rows,
                                                   uint32_t upr, uint32_t lpr_log2)
{
    using T = typename MoveUnit<V>::type;
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t lpr = 1u << lpr_log2, rpg = (uint32_t)WAVE >> lpr_log2;  // lanes per row, rows per group
    const uint32_t sub = lane >> lpr_log2, col0 = lane & (lpr - 1);
    const size_t pitch = (size_t)upr * V;
    const uint64_t n_groups = ((uint64_t)rows + rpg - 1) >> (6 - lpr_log2);
    const uint64_t wave = (uint64_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const uint64_t step = (uint64_t)gridDim.x * 4 * MOVE_U;
    for (uint64_t g0 = wave * MOVE_U; g0 < n_groups; g0 += step) {
        const uint64_t r_first = g0 * rpg;
        const uint64_t r_end = (g0 + MOVE_U) * rpg;
        const uint32_t r_last = (uint32_t)(r_end < rows ? r_end : rows) - 1;
        const uint32_t cf = move_shift(keys, c_lo, c_hi, dst_begin + (uint32_t)r_first);
        const uint32_t cl = move_shift(keys, cf, c_hi, dst_begin + r_last);
        const T* sp[MOVE_U];
        T* dp[MOVE_U];
#pragma unroll
        for (int j = 0; j < MOVE_U; ++j) {
            // past the segment's end: the lane moves the last row once more (the same bytes to the same place, and that
            // place is no source of this launch), which keeps every load and store of the trip unpredicated
            const uint64_t r_lane = (g0 + j) * rpg + sub;
            const uint64_t r = r_lane < rows ? r_lane : r_last;
            const uint32_t d = dst_begin + (uint32_t)r;
            const uint32_t c = cf == cl ? cf : move_shift(keys, cf, cl, d);
            sp[j] = reinterpret_cast<const T*>(src_base + ((size_t)d + c) * pitch);
            dp[j] = reinterpret_cast<T*>(dst + (size_t)r * pitch);
        }
        for (uint32_t col = col0; col < upr; col += lpr) {
            T v[MOVE_U];
#pragma unroll
            for (int j = 0; j < MOVE_U; ++j) v[j] = sp[j][col];
#pragma unroll
            for (int j = 0; j < MOVE_U; ++j) dp[j][col] = v[j];
        }
    }
}

template <typename F>
hipError_t dispatch_metric(int metric, F&& f)
{
    switch (metric) {
    case COSINE: return f(std::integral_constant<int, COSINE>{});
    case EUCLIDEAN: return f(std::integral_constant<int, EUCLIDEAN>{});
    case MANHATTAN: return f(std::integral_constant<int, MANHATTAN>{});
    case DOT: return f(std::integral_constant<int, DOT>{});
    default: return hipErrorInvalidValue;
    }
}

int env_int(const char* name, int dflt)
{
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
hipError_t launch_embed_f32(hipStream_t s, const float* emb, uint64_t n, uint32_t dim, bool normalize, double* out)
{
    if (n == 0 || dim == 0) return hipSuccess;
    if (n <= 16384 && dim <= EMBED_ROW_MAX) {  // a batch of queries, a small add: one wave per row
        hipLaunchKernelGGL(k_embed_f32_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, emb, n, dim, normalize ? 1 : 0, out);
        return hipGetLastError();
    }
    const uint64_t blocks = ((n + WAVE - 1) / WAVE + 3) / 4;
    const int grid = (int)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(k_embed_f32, dim3(grid), dim3(256), 0, s, emb, n, dim, normalize ? 1 : 0, out);
    return hipGetLastError();
}

hipError_t launch_ingest(hipStream_t s, const double* master, float* slab, float* inv_norm, uint8_t* flags,
                         IngestStats* stats, uint64_t n, uint32_t dim, uint32_t ld)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 3) / 4;
    const int grid = (int)(blocks < 8192 ? blocks : 8192);
    hipLaunchKernelGGL(k_ingest, dim3(grid), dim3(256), 0, s, master, slab, inv_norm, flags, stats, n, dim, ld);
    return hipGetLastError();
}

hipError_t launch_update_rows(hipStream_t s, const double* staged, const uint32_t* pos, uint32_t m, double* master, float* slab,
                              float* inv_norm, uint8_t* flags, uint8_t* out_flags, IngestStats* stats, uint32_t dim, uint32_t ld)
{
    if (m == 0) return hipSuccess;
    const uint32_t blocks = (m + 3) / 4;
    const dim3 grid(blocks < 8192 ? blocks : 8192);
    const uintptr_t both = reinterpret_cast<uintptr_t>(staged) | reinterpret_cast<uintptr_t>(master);
    if (dim % 2 == 0 && both % 16 == 0)
        hipLaunchKernelGGL(k_update_rows<16>, grid, dim3(256), 0, s, staged, pos, m, master, slab, inv_norm, flags, out_flags, stats,
                           dim, ld);
    else
        hipLaunchKernelGGL(k_update_rows<8>, grid, dim3(256), 0, s, staged, pos, m, master, slab, inv_norm, flags, out_flags, stats,
                           dim, ld);
    return hipGetLastError();
}

hipError_t launch_move_rows(hipStream_t s, const void* src_base, void* dst, uint64_t pitch, const uint32_t* keys, uint32_t c_lo,
                            uint32_t c_hi, uint64_t dst_begin, uint64_t rows)
{
    if (rows == 0 || pitch == 0) return hipSuccess;
    if (dst_begin + rows + c_hi > 0xFFFFFFFFull || pitch > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uintptr_t both = reinterpret_cast<uintptr_t>(src_base) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)pitch;
    const int v = both % 16 == 0 ? 16 : both % 8 == 0 ? 8 : both % 4 == 0 ? 4 : 1;
    const uint32_t upr = (uint32_t)(pitch / (uint64_t)v);
    uint32_t lpr_log2 = 0;  // lanes per row: the power of two that covers a row's units, a whole wave at most
    while (lpr_log2 < 6 && (1u << lpr_log2) < upr) ++lpr_log2;
    const uint64_t n_groups = (rows + (64u >> lpr_log2) - 1) >> (6 - lpr_log2);
    const uint64_t blocks = ((n_groups + MOVE_U - 1) / MOVE_U + 3) / 4;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    const char* sb = static_cast<const char*>(src_base);
    char* db = static_cast<char*>(dst);
    switch (v) {
    case 16: hipLaunchKernelGGL(k_move_rows<16>, grid, dim3(256), 0, s, sb, db, keys, c_lo, c_hi, (uint32_t)dst_begin, (uint32_t)rows, upr, lpr_log2); break;
    case 8: hipLaunchKernelGGL(k_move_rows<8>, grid, dim3(256), 0, s, sb, db, keys, c_lo, c_hi, (uint32_t)dst_begin, (uint32_t)rows, upr, lpr_log2); break;
    case 4: hipLaunchKernelGGL(k_move_rows<4>, grid, dim3(256), 0, s, sb, db, keys, c_lo, c_hi, (uint32_t)dst_begin, (uint32_t)rows, upr, lpr_log2); break;
    default: hipLaunchKernelGGL(k_move_rows<1>, grid, dim3(256), 0, s, sb, db, keys, c_lo, c_hi, (uint32_t)dst_begin, (uint32_t)rows, upr, lpr_log2); break;
    }
    return hipGetLastError();
}

namespace {
// lanes per row for a row of ld4 float4 (generic kernel)
int lanes_per_row(uint32_t ld4)
{
    int g = 1;
    while (g < 64 && (uint32_t)(g * 2) <= ld4) g *= 2;
    return g;
}

// Compiled (G lanes per row, VPL float4 per lane, U row groups in flight, BPC workgroups per CU)
// instantiations of k_scan.  The first entry whose G*VPL equals ld4 is the default; VL_SCAN_G /
// VL_SCAN_U / VL_SCAN_GRID pick another shape (tuning only).  Measured on MI355X at N=10M, dim=384
// (profiles/r01_tune_scan.txt): 12 x 16-byte loads in flight per lane and 3 workgroups per CU
// (12 waves, ~144 KB in flight per CU) stream at 7.17 TB/s; more resident waves were slower.
#define VL_SCAN_VARIANTS(X)                                                                         \
    X(8, 4, 3, 3) X(8, 8, 2, 3) X(8, 12, 1, 3) X(8, 16, 1, 3) X(16, 12, 1, 3) X(16, 16, 1, 3)       \
    X(16, 24, 1, 2) X(32, 1, 8, 4) X(32, 2, 4, 4) X(32, 4, 2, 4) X(32, 8, 1, 4) X(32, 12, 1, 3)      \
    X(32, 3, 2, 4) X(32, 3, 4, 3) X(16, 6, 1, 4) X(16, 6, 2, 1) X(8, 12, 2, 1) X(4, 24, 1, 2)        \
    X(32, 6, 1, 4) X(32, 6, 2, 3) X(16, 12, 2, 1) X(8, 24, 1, 2) X(64, 3, 2, 4) X(64, 3, 4, 3)       \
    X(16, 2, 4, 4) X(8, 4, 4, 3) X(16, 4, 2, 4) X(16, 4, 3, 3) X(8, 8, 1, 4) X(16, 8, 1, 4)          \
    X(16, 8, 2, 2)

struct ScanShape {
    bool special;
    int g, vpl, u, bpc;
};

constexpr int SCAN_TABLE[][4] = {
#define VL_ROW(G, VPL, U, BPC) {G, VPL, U, BPC},
    VL_SCAN_VARIANTS(VL_ROW)
#undef VL_ROW
};
constexpr int SCAN_TABLE_N = (int)(sizeof(SCAN_TABLE) / sizeof(SCAN_TABLE[0]));

// the default entry of a stride: the first one with that G * VPL; -1: the stride is not specialised
constexpr int default_scan_entry(uint32_t ld4)
{
    for (int i = 0; i < SCAN_TABLE_N; ++i)
        if ((uint32_t)(SCAN_TABLE[i][0] * SCAN_TABLE[i][1]) == ld4) return i;
    return -1;
}

constexpr bool is_default_scan_shape(int g, int vpl, int u)
{
    const int i = default_scan_entry((uint32_t)(g * vpl));
    return i >= 0 && SCAN_TABLE[i][0] == g && SCAN_TABLE[i][1] == vpl && SCAN_TABLE[i][2] == u;
}

ScanShape scan_shape_at(int i, uint32_t ld4)
{
    if (i < 0) return {false, lanes_per_row(ld4), 0, 1, 4};  // the generic kernel
    return {true, SCAN_TABLE[i][0], SCAN_TABLE[i][1], SCAN_TABLE[i][2], SCAN_TABLE[i][3]};
}

// The shape the subset and range scans run, and k_scan unless a tuning variable picks another: with it a row's key is
// the same in all three.
ScanShape default_scan_shape(uint32_t ld4) { return scan_shape_at(default_scan_entry(ld4), ld4); }

// k_scan's shape: the default one, or the entry VL_SCAN_G / VL_SCAN_U name
ScanShape scan_shape(uint32_t ld4)
{
    const int want_g = env_int("VL_SCAN_G", 0), want_u = env_int("VL_SCAN_U", 0);
    int pick = default_scan_entry(ld4);
    for (int i = pick; i >= 0 && i < SCAN_TABLE_N; ++i) {
        if ((uint32_t)(SCAN_TABLE[i][0] * SCAN_TABLE[i][1]) != ld4) continue;
        if (want_g && SCAN_TABLE[i][0] == want_g && (!want_u || SCAN_TABLE[i][2] == want_u)) {
            pick = i;
            break;
        }
        if (!want_g && want_u && SCAN_TABLE[i][2] == want_u && SCAN_TABLE[i][0] == SCAN_TABLE[pick][0]) {
            pick = i;
            break;
        }
    }
    return scan_shape_at(pick, ld4);
}
}  // namespace

namespace {
// Workgroups of `kernel` (256 threads, no dynamic LDS) that are resident at once on this device:
// the scan is one persistent wave of workgroups that grid-stride over the rows, so every CU streams
// for the whole launch and no second, partially filled round of workgroups trails behind.
int resident_blocks(const void* kernel, int* n_cus)
{
    struct Entry {
        const void* k;
        int dev;
        int blocks;
        int cus;
    };
    static Entry cache[256];
    static int n_cache = 0;
    static std::mutex mu;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    for (int i = 0; i < n_cache; ++i)
        if (cache[i].k == kernel && cache[i].dev == dev) {
            *n_cus = cache[i].cus;
            return cache[i].blocks;
        }
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu <= 0) per_cu = 4;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    // the occupancy API can over-report by one block per CU (MI355X_MICROARCH.md): stay one below 8
    if (per_cu > 7) per_cu = 7;
    const int blocks = per_cu * cus;
    if (n_cache < 256) cache[n_cache++] = {kernel, dev, blocks, cus};
    *n_cus = cus;
    return blocks;
}

int scan_grid(uint64_t n, const ScanShape& sh, const void* kernel)
{
    const uint64_t rps = 64 / sh.g;
    const uint64_t steps = (n + rps - 1) / rps;
    const uint64_t per_block = 4ull * sh.u;
    uint64_t blocks = (steps + per_block - 1) / per_block;
    uint64_t cap = (uint64_t)env_int("VL_SCAN_GRID", 0);
    if (cap == 0) {
        int cus = 0;
        const uint64_t resident = (uint64_t)resident_blocks(kernel, &cus);
        cap = (uint64_t)sh.bpc * (uint64_t)cus;
        if (cap > resident) cap = resident;
    }
    if (blocks > cap) blocks = cap;
    if (blocks > (uint64_t)SCAN_MAX_GRID) blocks = SCAN_MAX_GRID;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}
}  // namespace

#ifdef VL_DBG_STAMPS
extern "C" int vl_dbg_read_stamps(unsigned long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(vl_dbg_stamps), sizeof(unsigned long long) * 32);
}
#endif

namespace {
// One f32 scan family = three kernels (kernel-argument query, f64 query in device memory, run-time stride) whose
// argument lists are  head..., [q64, dim,] n, [ld4,] tail..., [qa]:  `head` / `tail` are what the family puts in front
// of and behind the arguments every scan takes.  A family names its kernels and says
//   ALL_SHAPES         every VL_SCAN_VARIANTS entry is compiled (k_scan: the tuning variables can pick any), or only
//                      the default entry of each stride
//   Q64_AT_ANY_STRIDE  the q64 form exists at every specialised stride (k_scan: the k > 60 multi-list path passes no
//                      host query), or only at strides past the kernel-argument query
template <int MM>
struct TopFamily {
    static constexpr bool ALL_SHAPES = true, Q64_AT_ANY_STRIDE = true;
    template <int G, int VPL, int U> static auto qarg() { return k_scan<MM, G, VPL, U>; }
    template <int G, int VPL, int U> static auto q64() { return k_scan_q64<MM, G, VPL, U>; }
    template <int G> static auto generic() { return k_scan_generic<MM, G>; }
};
template <int MM>
struct SubsetFamily {
    static constexpr bool ALL_SHAPES = false, Q64_AT_ANY_STRIDE = false;
    template <int G, int VPL, int U> static auto qarg() { return k_scan_subset<MM, G, VPL, U>; }
    template <int G, int VPL, int U> static auto q64() { return k_scan_subset_q64<MM, G, VPL, U>; }
    template <int G> static auto generic() { return k_scan_subset_generic<MM, G>; }
};
template <int MM, bool SUBSET>
struct RangeFamily {
    static constexpr bool ALL_SHAPES = false, Q64_AT_ANY_STRIDE = false;
    template <int G, int VPL, int U> static auto qarg() { return k_scan_range<MM, G, VPL, U, SUBSET>; }
    template <int G, int VPL, int U> static auto q64() { return k_scan_range_q64<MM, G, VPL, U, SUBSET>; }
    template <int G> static auto generic() { return k_scan_range_generic<MM, G, SUBSET>; }
};

template <int MM, bool SUBSET>
struct GroupBestFamily {
    static constexpr bool ALL_SHAPES = false, Q64_AT_ANY_STRIDE = false;
    template <int G, int VPL, int U> static auto qarg() { return k_scan_group_best<MM, G, VPL, U, SUBSET>; }
    template <int G, int VPL, int U> static auto q64() { return k_scan_group_best_q64<MM, G, VPL, U, SUBSET>; }
    template <int G> static auto generic() { return k_scan_group_best_generic<MM, G, SUBSET>; }
};

// does a scan of this shape and stride take its query in the kernel arguments
bool shape_takes_qarg(const ScanShape& sh, uint32_t ld, const float* q32_host)
{
    return q32_host != nullptr && sh.special && ld <= (uint32_t)SCAN_QARG_FLOATS;
}

// shape match -> kernel-argument or q64 form -> scan_grid -> launch
template <class Fam, class Head, class Tail>
hipError_t launch_scan_family(hipStream_t s, const ScanShape& sh, uint64_t n, uint32_t ld, const double* q64, uint32_t dim,
                              const float* q32_host, const Head& head, const Tail& tail, int* grid)
{
    const uint32_t n32 = (uint32_t)n, ld4 = ld / 4;
    const bool qarg = shape_takes_qarg(sh, ld, q32_host);
    auto launch = [&](auto kern, const auto& mid, const auto& last) {
        *grid = scan_grid(n, sh, reinterpret_cast<const void*>(kern));
        std::apply([&](const auto&... a) { hipLaunchKernelGGL(kern, dim3(*grid), dim3(256), 0, s, a...); },
                   std::tuple_cat(head, mid, tail, last));
    };
    if (sh.special) {
        bool launched = false;
#define VL_TRY_VARIANT(G, VPL, U, BPC)                                                                      \
    if constexpr (Fam::ALL_SHAPES || is_default_scan_shape(G, VPL, U)) {                                    \
        if (!launched && sh.g == G && sh.vpl == VPL && sh.u == U) {                                         \
            if constexpr (G * VPL * 4 <= SCAN_QARG_FLOATS) {                                                \
                if (qarg) {                                                                                 \
                    ScanQArg qa;                                                                            \
                    memcpy(qa.v, q32_host, (size_t)ld * sizeof(float));                                     \
                    launch(Fam::template qarg<G, VPL, U>(), std::make_tuple(n32), std::make_tuple(qa));     \
                    launched = true;                                                                        \
                }                                                                                           \
            }                                                                                               \
            if constexpr (Fam::Q64_AT_ANY_STRIDE || G * VPL * 4 > SCAN_QARG_FLOATS) {                       \
                if (!launched) {                                                                            \
                    launch(Fam::template q64<G, VPL, U>(), std::make_tuple(q64, dim, n32), std::tuple<>()); \
                    launched = true;                                                                        \
                }                                                                                           \
            }                                                                                               \
        }                                                                                                   \
    }
        VL_SCAN_VARIANTS(VL_TRY_VARIANT)
#undef VL_TRY_VARIANT
        if (!launched) return hipErrorInvalidValue;  // a kernarg-sized stride without its query there
    } else {
#define VL_SCAN_GEN(G) \
    case G: launch(Fam::template generic<G>(), std::make_tuple(q64, dim, n32, ld4), std::tuple<>()); break;
        switch (sh.g) {
            VL_SCAN_GEN(1)
            VL_SCAN_GEN(2)
            VL_SCAN_GEN(4)
            VL_SCAN_GEN(8)
            VL_SCAN_GEN(16)
            VL_SCAN_GEN(32)
            VL_SCAN_GEN(64)
        default: return hipErrorInvalidValue;
        }
#undef VL_SCAN_GEN
    }
    return hipGetLastError();
}
}  // namespace

bool scan_takes_qarg(uint32_t ld)
{
    if ((ld & 3) || ld > (uint32_t)SCAN_QARG_FLOATS) return false;
    return default_scan_shape(ld / 4).special;
}

hipError_t launch_scan(hipStream_t s, int metric, const float* slab, const float* inv_norm, const double* q64,
                       uint64_t n, uint32_t dim, uint32_t ld, Cand32* partials, ScanPlan* plan, const float* q32_host)
{
    if (n == 0 || n >= 0xFFFFFFFFull || (ld & 3)) return hipErrorInvalidValue;
    const ScanShape sh = scan_shape(ld / 4);
    const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
    if (!shape_takes_qarg(sh, ld, q32_host) && !q64) return hipErrorInvalidValue;
    int grid = 0;
    hipError_t rc = dispatch_metric(metric, [&](auto M) -> hipError_t {
        return launch_scan_family<TopFamily<decltype(M)::value>>(s, sh, n, ld, q64, dim, q32_host,
                                                                 std::make_tuple(slab4, inv_norm), std::make_tuple(partials), &grid);
    });
    if (plan) {
        plan->grid = grid;
        plan->variant = sh.special ? (sh.g * 10000 + sh.vpl * 100 + sh.u) : -sh.g;
    }
    return rc;
}

// Batch shapes: one (G, VPL) per supported row length, QB = 8 queries per pass.
// (lanes per row, 16-byte chunks per lane): row strides 32, 64, 96, 128, 192, 256, 320, 384, 512, 640, 768, 1024, 1536 floats.
// The first shape whose G * VPL matches the stride runs.  Strides 32 and 64 take FOUR lanes per row (16 rows per wave step):
// at such lengths a (row, query) pair is ~35 instructions of which 19 are the cross-lane reduction, the key compare, the
// ballot and the branch -- per ROW costs that 16 rows per step halve (round 4, `tools/manhattan_probe.py`).
#define VL_BATCH_SHAPES(X) X(4, 2) X(4, 4) X(8, 3) X(8, 4) X(8, 6) X(8, 8) X(8, 10) X(8, 12) X(8, 16) X(16, 10) X(16, 12) X(16, 16) X(16, 24)

bool scan_batch_supported(uint32_t ld)
{
    const uint32_t ld4 = ld / 4;
    bool ok = false;
#define VL_CHK(G, VPL) ok = ok || ((uint32_t)(G * VPL) == ld4);
    VL_BATCH_SHAPES(VL_CHK)
#undef VL_CHK
    return ok && (ld % 4) == 0;
}

hipError_t launch_scan_batch(hipStream_t s, int metric, const float* slab, const float* inv_norm, const double* q64,
                             uint32_t nq, uint64_t n, uint32_t dim, uint32_t ld, Cand32* partials, ScanPlan* plan)
{
    if (n == 0 || n >= 0xFFFFFFFFull || (ld & 3) || nq == 0 || nq > (uint32_t)SCAN_BATCH_MAX_QUERIES) return hipErrorInvalidValue;
    const uint32_t ld4 = ld / 4;
    const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
    const uint32_t n32 = (uint32_t)n;
    const uint32_t groups = (nq + SCAN_BATCH_QB - 1) / SCAN_BATCH_QB;
    int grid = 0;
    hipError_t rc = dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        bool launched = false;
#define VL_TRY_BATCH(G, VPL)                                                                                  \
    if (!launched && (uint32_t)(G * VPL) == ld4) {                                                            \
        auto kern = k_scan_batch<MM, G, VPL, SCAN_BATCH_QB>;                                                  \
        int cus = 0;                                                                                          \
        const int resident = resident_blocks(reinterpret_cast<const void*>(kern), &cus);                      \
        const uint64_t steps = (n + (64 / G) - 1) / (64 / G);                                                 \
        uint64_t blocks = (steps + 3) / 4;                                                                    \
        uint64_t cap = (uint64_t)env_int("VL_BATCH_GRID", 0);                                                 \
        if (cap == 0) cap = (uint64_t)resident;                                                               \
        if (cap > (uint64_t)SCAN_BATCH_MAX_GRID) cap = SCAN_BATCH_MAX_GRID;                                   \
        if (groups > 1) {                                                                                     \
            /* several groups in one launch: the resident workgroups are shared out over them, every query's */ \
            /* lists must fit the finalize kernel without a merge level (<= 64) and the partial-list buffer */  \
            cap = std::max<uint64_t>(1, cap / groups);                                                        \
            cap = std::min<uint64_t>(cap, 64);                                                                \
            cap = std::min<uint64_t>(cap, std::max<uint64_t>(1, PARTIALS32_LISTS / ((uint64_t)groups * SCAN_BATCH_QB))); \
        }                                                                                                     \
        if (blocks > cap) blocks = cap;                                                                       \
        grid = (int)(blocks < 1 ? 1 : blocks);                                                                \
        hipLaunchKernelGGL(kern, dim3(grid, groups), dim3(256), 0, s, slab4, inv_norm, q64, nq, dim, n32, partials); \
        launched = true;                                                                                      \
    }
        VL_BATCH_SHAPES(VL_TRY_BATCH)
#undef VL_TRY_BATCH
        if (!launched) return hipErrorInvalidValue;
        return hipGetLastError();
    });
    if (plan) {
        plan->grid = grid;
        plan->variant = 0;
    }
    return rc;
}

namespace {
// Reduce n_lists sorted lists per query to <= 64 with merge levels.  `scratch` holds two ping-pong
// regions of nq x 64 lists.  Returns the final list array, count and per-query stride.
template <typename K, typename C>
const C* reduce_lists(hipStream_t s, const C* lists, int* n_lists, size_t* stride_q, int nq, C* scratch)
{
    int n = *n_lists;
    size_t in_stride = *stride_q;
    int ping = 0;
    while (n > 64) {
        const int blocks = (n + 63) / 64;
        const size_t out_stride = (size_t)64 * KP;
        C* out = scratch + (size_t)ping * nq * out_stride;
        hipLaunchKernelGGL((k_merge_lists<K, C>), dim3(blocks, nq), dim3(1024), 0, s, lists, n, in_stride, out,
                           out_stride);
        lists = out;
        in_stride = out_stride;
        n = blocks;
        ping ^= 1;
    }
    *n_lists = n;
    *stride_q = in_stride;
    return lists;
}
}  // namespace

hipError_t launch_merge_finalize(hipStream_t s, int metric, Cand32* partials, int n_lists, int nq,
                                 const double* master, const double* q64, const double* q_norms, uint32_t dim,
                                 uint64_t n_rows, uint32_t k, double max_row_norm, SearchResultBlock* out,
                                 double in_extra, uint32_t seq, const ShardRecordSink* sink)
{
    if (seq && nq != 1) return hipErrorInvalidValue;
    const ShardRecordSink sk = sink ? *sink : ShardRecordSink{};
    const uint32_t ld = (dim + 3u) & ~3u;
    size_t stride = (size_t)n_lists * KP;
    const Cand32* lists = reduce_lists<float, Cand32>(s, partials, &n_lists, &stride, nq, partials + PARTIALS32_LISTS * KP);
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_merge_finalize<MM>), dim3(nq), dim3(1024), 0, s, lists, n_lists, stride, master, q64,
                           q_norms, dim, ld, n_rows, k, max_row_norm, in_extra, out, seq, sk);
        return hipGetLastError();
    });
}

hipError_t launch_batch_finalize(hipStream_t s, int metric, const Cand32* lists, int nq, const double* master, const double* q64,
                                 const double* q_norms, uint32_t dim, uint64_t n_rows, uint32_t k, double max_row_norm,
                                 SearchResultBlock* out, double in_extra, double* score_scratch, const ShardRecordSink* sink)
{
    if (nq <= 0 || !score_scratch) return hipErrorInvalidValue;
    const uint32_t ld = (dim + 3u) & ~3u;
    const ShardRecordSink sk = sink ? *sink : ShardRecordSink{};
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_batch_rescore<MM>), dim3((unsigned)nq * 4u), dim3(256), 0, s, lists, master, q64, dim, score_scratch);
        hipLaunchKernelGGL((k_batch_rank_emit<MM>), dim3(((unsigned)nq + 3u) / 4u), dim3(256), 0, s, lists, (const double*)score_scratch,
                           q_norms, (uint32_t)nq, ld, n_rows, k, max_row_norm, in_extra, out, sk);
        return hipGetLastError();
    });
}

hipError_t launch_batch_finalize_rows(hipStream_t s, int metric, const Cand32* lists, int nq, const double* master,
                                      const double* q64, const double* q_norms, uint32_t dim, const uint32_t* m_of,
                                      const uint32_t* k_of, double max_row_norm, SearchResultBlock* out, double in_extra,
                                      double* score_scratch)
{
    if (nq <= 0 || !score_scratch || !m_of || !k_of) return hipErrorInvalidValue;
    const uint32_t ld = (dim + 3u) & ~3u;
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_batch_rescore<MM>), dim3((unsigned)nq * 4u), dim3(256), 0, s, lists, master, q64, dim, score_scratch);
        hipLaunchKernelGGL((k_batch_rank_emit_rows<MM>), dim3(((unsigned)nq + 3u) / 4u), dim3(256), 0, s, lists,
                           (const double*)score_scratch, q_norms, (uint32_t)nq, ld, m_of, k_of, max_row_norm, in_extra, out);
        return hipGetLastError();
    });
}

namespace {
// the MFMA filter's metrics: the collapse stage has no Manhattan form
template <typename F>
hipError_t dispatch_mfma_metric(int metric, F&& f)
{
    switch (metric) {
    case COSINE: return f(std::integral_constant<int, COSINE>{});
    case EUCLIDEAN: return f(std::integral_constant<int, EUCLIDEAN>{});
    case DOT: return f(std::integral_constant<int, DOT>{});
    default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t launch_batch_rank_collapse(hipStream_t s, int metric, const Cand32* lists, const double* scores, int nq,
                                      const double* q_norms, uint32_t ld, uint64_t n_rows, uint32_t k, double max_row_norm,
                                      const uint32_t* group_of_row, uint64_t index_rows, GroupedResultBlock* out, double in_extra)
{
    if (nq <= 0 || !lists || !scores || !q_norms || !group_of_row || !out || n_rows == 0 || k == 0 || k > (uint32_t)KFAST_MAX ||
        index_rows >= 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    return dispatch_mfma_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_batch_rank_collapse<MM>), dim3(((unsigned)nq + 3u) / 4u), dim3(256), 0, s, lists, scores, q_norms,
                           (uint32_t)nq, ld, n_rows, k, max_row_norm, in_extra, group_of_row, (uint32_t)index_rows, out);
        return hipGetLastError();
    });
}

hipError_t launch_batch_finalize_grouped(hipStream_t s, int metric, const Cand32* lists, int nq, const double* master,
                                         const double* q64, const double* q_norms, uint32_t dim, uint64_t n_rows, uint32_t k,
                                         double max_row_norm, const uint32_t* group_of_row, uint64_t index_rows,
                                         GroupedResultBlock* out, double in_extra, double* score_scratch)
{
    if (nq <= 0 || !score_scratch) return hipErrorInvalidValue;
    const uint32_t ld = (dim + 3u) & ~3u;
    const hipError_t e = dispatch_mfma_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_batch_rescore<MM>), dim3((unsigned)nq * 4u), dim3(256), 0, s, lists, master, q64, dim, score_scratch);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    return launch_batch_rank_collapse(s, metric, lists, score_scratch, nq, q_norms, ld, n_rows, k, max_row_norm, group_of_row,
                                      index_rows, out, in_extra);
}

hipError_t launch_batch_rescore(hipStream_t s, int metric, const Cand32* lists, int nq, const double* master, const double* q64,
                                uint32_t dim, double* scores)
{
    if (nq <= 0 || !lists || !master || !q64 || !scores) return hipErrorInvalidValue;
    return dispatch_mfma_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_batch_rescore<MM>), dim3((unsigned)nq * 4u), dim3(256), 0, s, lists, master, q64, dim, scores);
        return hipGetLastError();
    });
}

hipError_t launch_merge_finalize_multi(hipStream_t s, int metric, Cand32* partials, int n_lists_total, int n_parts,
                                       const double* master, const double* q64, const double* q_norm, uint32_t dim,
                                       uint64_t n_rows, uint32_t k, double max_row_norm, SearchResultBlock* out)
{
    if (n_parts < 2 || n_parts > KMULTI_PARTS || n_lists_total % n_parts != 0) return hipErrorInvalidValue;
    const uint32_t ld = (dim + 3u) & ~3u;
    int n_lists = n_lists_total / n_parts;  // consecutive workgroup lists form one partition
    size_t stride = (size_t)n_lists * KP;
    const Cand32* lists = reduce_lists<float, Cand32>(s, partials, &n_lists, &stride, n_parts, partials + PARTIALS32_LISTS * KP);
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_merge_finalize_multi<MM>), dim3(1), dim3(1024), 0, s, lists, n_lists, stride, n_parts, master,
                           q64, q_norm, dim, ld, n_rows, k, max_row_norm, out);
        return hipGetLastError();
    });
}

hipError_t launch_exact_scan(hipStream_t s, int metric, const double* master, const double* q64, uint64_t n,
                             uint32_t dim, double* scores, uint32_t* nan_flag)
{
    if (n == 0) return hipSuccess;
    const uint64_t tiles = (n + EX_ROWS - 1) / EX_ROWS;
    const int grid = (int)(tiles < 4096 ? tiles : 4096);
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_exact_scan<MM>), dim3(grid), dim3(256), 0, s, master, q64, n, dim, scores, nan_flag);
        return hipGetLastError();
    });
}

hipError_t launch_exact_scan_subset(hipStream_t s, int metric, const double* master, const double* q64, const uint32_t* plist,
                                    uint64_t m, uint32_t dim, double* scores, uint32_t* nan_flag)
{
    if (m == 0) return hipSuccess;
    const uint64_t tiles = (m + EX_ROWS - 1) / EX_ROWS;
    const int grid = (int)(tiles < 4096 ? tiles : 4096);
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_exact_scan_subset<MM>), dim3(grid), dim3(256), 0, s, master, q64, plist, m, dim, scores, nan_flag);
        return hipGetLastError();
    });
}

// The subset scan runs the default shape of every stride VL_SCAN_VARIANTS specialises, so that a row's key is k_scan's;
// other strides take the generic kernel with k_scan_generic's lanes per row.
bool scan_subset_takes_qarg(uint32_t ld) { return scan_takes_qarg(ld); }

hipError_t launch_scan_subset(hipStream_t s, int metric, const float* slab, const float* inv_norm, const uint32_t* plist,
                              uint64_t m, const double* q64, uint32_t dim, uint32_t ld, Cand32* partials, ScanPlan* plan,
                              const float* q32_host)
{
    if (m == 0 || m >= 0xFFFFFFFFull || (ld & 3)) return hipErrorInvalidValue;
    const ScanShape sh = default_scan_shape(ld / 4);
    const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
    if (!shape_takes_qarg(sh, ld, q32_host) && !q64) return hipErrorInvalidValue;
    int grid = 0;
    hipError_t rc = dispatch_metric(metric, [&](auto M) -> hipError_t {
        return launch_scan_family<SubsetFamily<decltype(M)::value>>(s, sh, m, ld, q64, dim, q32_host,
                                                                    std::make_tuple(slab4, inv_norm, plist),
                                                                    std::make_tuple(partials), &grid);
    });
    if (plan) {
        plan->grid = grid;
        plan->variant = sh.special ? (SUBSET_VARIANT_BASE + sh.g * 10000 + sh.vpl * 100 + sh.u) : -(SUBSET_VARIANT_BASE + sh.g);
    }
    return rc;
}

// The masked scan: the default shape of a stride VL_SCAN_VARIANTS specialises (scan_masked_supported(ld)), the query as
// launch_scan_subset takes it; the grid is k_scan's, sized from n.
bool scan_masked_supported(uint32_t ld) { return !(ld & 3) && default_scan_shape(ld / 4).special; }

hipError_t launch_scan_masked(hipStream_t s, int metric, const float* slab, const float* inv_norm, const unsigned long long* keep,
                              uint64_t n, const double* q64, uint32_t dim, uint32_t ld, Cand32* partials, ScanPlan* plan,
                              const float* q32_host)
{
    if (n == 0 || n >= 0xFFFFFFFFull || !keep || !scan_masked_supported(ld)) return hipErrorInvalidValue;
    const ScanShape sh = default_scan_shape(ld / 4);
    const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
    const bool qarg = shape_takes_qarg(sh, ld, q32_host);
    if (!qarg && (!q64 || ld <= (uint32_t)SCAN_QARG_FLOATS)) return hipErrorInvalidValue;
    int grid = 0;
    hipError_t rc = dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        bool launched = false;
#define VL_TRY_VARIANT(G, VPL, U, BPC)                                                                                   \
    if constexpr (is_default_scan_shape(G, VPL, U)) {                                                                    \
        if (!launched && sh.g == G && sh.vpl == VPL && sh.u == U) {                                                      \
            if constexpr (G * VPL * 4 <= SCAN_QARG_FLOATS) {                                                             \
                ScanQArg qa;                                                                                             \
                memcpy(qa.v, q32_host, (size_t)ld * sizeof(float));                                                      \
                grid = scan_grid(n, sh, reinterpret_cast<const void*>(k_scan_masked<MM, G, VPL, U>));                    \
                hipLaunchKernelGGL((k_scan_masked<MM, G, VPL, U>), dim3(grid), dim3(256), 0, s, slab4, inv_norm, keep,   \
                                   (uint32_t)n, partials, qa);                                                           \
            } else {                                                                                                     \
                grid = scan_grid(n, sh, reinterpret_cast<const void*>(k_scan_masked_q64<MM, G, VPL, U>));                \
                hipLaunchKernelGGL((k_scan_masked_q64<MM, G, VPL, U>), dim3(grid), dim3(256), 0, s, slab4, inv_norm,     \
                                   keep, q64, dim, (uint32_t)n, partials);                                               \
            }                                                                                                            \
            launched = true;                                                                                             \
        }                                                                                                                \
    }
        VL_SCAN_VARIANTS(VL_TRY_VARIANT)
#undef VL_TRY_VARIANT
        return launched ? hipGetLastError() : hipErrorInvalidValue;
    });
    if (plan) {
        plan->grid = grid;
        plan->variant = MASK_VARIANT_BASE + sh.g * 10000 + sh.vpl * 100 + sh.u;
    }
    return rc;
}

namespace {
// The jobs scan of a shape: fn(kernel, std::true_type) for the stride's default shape, fn(kernel, std::false_type) for the
// generic kernel (which takes ld4 as well).
template <int MM, class Fn>
hipError_t with_subset_jobs_kernel(const ScanShape& sh, Fn&& fn)
{
    if (sh.special) {
#define VL_TRY_VARIANT(G, VPL, U, BPC)                                                                                  \
    if constexpr (is_default_scan_shape(G, VPL, U)) {                                                                   \
        if (sh.g == G && sh.vpl == VPL && sh.u == U) return fn(k_scan_subset_jobs<MM, G, VPL, U>, std::true_type{});    \
    }
        VL_SCAN_VARIANTS(VL_TRY_VARIANT)
#undef VL_TRY_VARIANT
        return hipErrorInvalidValue;
    }
#define VL_SCAN_GEN(G) \
    case G: return fn(k_scan_subset_jobs_generic<MM, G>, std::false_type{});
    switch (sh.g) {
        VL_SCAN_GEN(1)
        VL_SCAN_GEN(2)
        VL_SCAN_GEN(4)
        VL_SCAN_GEN(8)
        VL_SCAN_GEN(16)
        VL_SCAN_GEN(32)
        VL_SCAN_GEN(64)
    default: return hipErrorInvalidValue;
    }
#undef VL_SCAN_GEN
}
}  // namespace

hipError_t scan_subset_jobs_shape(int metric, uint32_t ld, int* g, int* u, int* resident)
{
    if ((ld & 3) || ld == 0) return hipErrorInvalidValue;
    const ScanShape sh = default_scan_shape(ld / 4);
    *g = sh.g;
    *u = sh.u;
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        return with_subset_jobs_kernel<decltype(M)::value>(sh, [&](auto kern, auto) -> hipError_t {
            // scan_grid's cap for this kernel
            uint64_t cap = (uint64_t)env_int("VL_SCAN_GRID", 0);
            if (cap == 0) {
                int cus = 0;
                const uint64_t res = (uint64_t)resident_blocks(reinterpret_cast<const void*>(kern), &cus);
                cap = std::min<uint64_t>((uint64_t)sh.bpc * (uint64_t)cus, res);
            }
            *resident = (int)std::max<uint64_t>(1, std::min<uint64_t>(cap, (uint64_t)SCAN_MAX_GRID));
            return hipSuccess;
        });
    });
}

hipError_t launch_scan_subset_jobs(hipStream_t s, int metric, const float* slab, const float* inv_norm, const SubsetJobDev* jobs,
                                   uint32_t n_jobs, uint32_t gx, const double* q64, uint32_t dim, uint32_t ld, Cand32* partials,
                                   ScanPlan* plan)
{
    if (n_jobs == 0 || n_jobs > (uint32_t)SCAN_BATCH_MAX_QUERIES || gx == 0 || (uint64_t)gx * n_jobs > PARTIALS32_LISTS ||
        (ld & 3) || ld == 0 || !jobs || !q64)
        return hipErrorInvalidValue;
    const ScanShape sh = default_scan_shape(ld / 4);
    const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
    const hipError_t rc = dispatch_metric(metric, [&](auto M) -> hipError_t {
        return with_subset_jobs_kernel<decltype(M)::value>(sh, [&](auto kern, auto special) -> hipError_t {
            if constexpr (decltype(special)::value)
                hipLaunchKernelGGL(kern, dim3(gx, n_jobs), dim3(256), 0, s, slab4, inv_norm, jobs, q64, dim, partials);
            else
                hipLaunchKernelGGL(kern, dim3(gx, n_jobs), dim3(256), 0, s, slab4, inv_norm, jobs, q64, dim, ld / 4, partials);
            return hipGetLastError();
        });
    });
    if (plan) {
        plan->grid = (int)gx;
        plan->variant = sh.special ? (SUBSET_JOBS_VARIANT_BASE + sh.g * 10000 + sh.vpl * 100 + sh.u) : -(SUBSET_JOBS_VARIANT_BASE + sh.g);
    }
    return rc;
}

hipError_t launch_merge_finalize_jobs(hipStream_t s, int metric, Cand32* partials, int n_lists, const SubsetJobDev* jobs,
                                      uint32_t n_jobs, const double* master, const double* q64, const double* q_norms,
                                      uint32_t dim, double max_row_norm, SearchResultBlock* out)
{
    if (n_jobs == 0 || n_lists <= 0 || (n_jobs > (uint32_t)SCAN_BATCH_QB && n_lists > 64) ||
        (uint64_t)n_lists * n_jobs > PARTIALS32_LISTS)
        return hipErrorInvalidValue;
    const uint32_t ld = (dim + 3u) & ~3u;
    size_t stride = (size_t)n_lists * KP;
    const Cand32* lists = reduce_lists<float, Cand32>(s, partials, &n_lists, &stride, (int)n_jobs, partials + PARTIALS32_LISTS * KP);
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_merge_finalize_jobs<MM>), dim3(n_jobs), dim3(1024), 0, s, lists, n_lists, stride, master, q64,
                           q_norms, dim, ld, jobs, max_row_norm, out);
        return hipGetLastError();
    });
}

int filter_grid_for(uint64_t n, uint32_t* chunk)
{
    // at least 4 tiles of 256 positions per workgroup, at most FILTER_MAX_GRID workgroups
    uint64_t c = (n + FILTER_MAX_GRID - 1) / FILTER_MAX_GRID;
    if (c < 1024) c = 1024;
    *chunk = (uint32_t)c;
    return (int)((n + c - 1) / c);
}

hipError_t launch_filter_count(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                               uint64_t nf, uint32_t* counts, uint32_t* m_out, bool invert)
{
    if (n == 0 || n >= 0xFFFFFFFFull || (nf == 0 && !invert) || nf >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    uint32_t chunk = 0;
    const int grid = filter_grid_for(n, &chunk);
    hipLaunchKernelGGL(k_filter_count, dim3(grid), dim3(256), 0, s, pos_ids, (uint32_t)n, fids, (uint32_t)nf, chunk, counts,
                       invert ? 1u : 0u);
    hipLaunchKernelGGL(k_filter_scan, dim3(1), dim3(FILTER_MAX_GRID), 0, s, counts, (uint32_t)grid, m_out);
    return hipGetLastError();
}

hipError_t launch_filter_scan(hipStream_t s, uint32_t* counts, uint32_t nb, uint32_t* m_out)
{
    if (nb == 0 || nb > (uint32_t)FILTER_MAX_GRID || !counts || !m_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_filter_scan, dim3(1), dim3(FILTER_MAX_GRID), 0, s, counts, nb, m_out);
    return hipGetLastError();
}

hipError_t launch_filter_compact(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                                 uint64_t nf, const uint32_t* offsets, uint64_t m, uint32_t* plist, bool invert)
{
    if (n == 0 || n >= 0xFFFFFFFFull || (nf == 0 && !invert) || nf >= 0xFFFFFFFFull || m == 0) return hipErrorInvalidValue;
    uint32_t chunk = 0;
    const int grid = filter_grid_for(n, &chunk);
    hipLaunchKernelGGL(k_filter_compact, dim3(grid), dim3(256), 0, s, pos_ids, (uint32_t)n, fids, (uint32_t)nf, chunk, offsets,
                       (uint32_t)m, plist, invert ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_filter_bits(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                              uint64_t nf, unsigned long long* keep, bool include)
{
    if (n == 0 || n >= 0xFFFFFFFFull || nf >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t n_words = (n + 63) / 64;
    const int grid = (int)std::min<uint64_t>((n_words + 3) / 4, FILTER_MAX_GRID);
    hipLaunchKernelGGL(k_filter_bits, dim3(grid), dim3(256), 0, s, pos_ids, (uint32_t)n, fids, (uint32_t)nf, (uint32_t)n_words, keep,
                       include ? 1u : 0u);
    return hipGetLastError();
}

int select_grid_for(uint64_t n)
{
    const uint64_t steps = (n + 63) / 64;
    uint64_t blocks = (steps + 3) / 4;
    if (blocks > (uint64_t)SELECT_MAX_GRID) blocks = SELECT_MAX_GRID;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

hipError_t launch_exact_select(hipStream_t s, const double* scores, uint64_t n, uint32_t k, Cand64* partials,
                               const uint32_t* nan_flag, SearchResultBlock* out, const SearchResultBlock* after)
{
    if (n == 0 || n >= 0xFFFFFFFFull || k > (uint32_t)KP) return hipErrorInvalidValue;
    const int grid = select_grid_for(n);
    hipLaunchKernelGGL(k_select64, dim3(grid), dim3(256), 0, s, scores, (uint32_t)n, after, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int n_lists = grid;
    size_t stride = (size_t)n_lists * KP;
    const Cand64* lists = reduce_lists<double, Cand64>(s, partials, &n_lists, &stride, 1, partials + (size_t)SELECT_MAX_GRID * KP);
    hipLaunchKernelGGL(k_merge64_emit, dim3(1), dim3(1024), 0, s, lists, n_lists, n, k, nan_flag, out);
    return hipGetLastError();
}

uint64_t sort_capacity_for(uint64_t n)
{
    uint64_t cap = SORT_LOCAL;
    while (cap < n) cap <<= 1;
    return cap;
}

namespace {
// ascending sort of cap (a power of two >= SORT_LOCAL) entries on (key, payload)
template <typename P>
void bitonic_network(hipStream_t s, unsigned long long* ok, P* opos, uint64_t cap)
{
    const int lgrid = (int)(cap / SORT_LOCAL);
    // k = 2 .. SORT_LOCAL entirely in LDS
    hipLaunchKernelGGL((k_bitonic_local<P>), dim3(lgrid), dim3(1024), 0, s, ok, opos, (uint64_t)2, (uint64_t)SORT_LOCAL);
    for (uint64_t kk = (uint64_t)SORT_LOCAL << 1; kk <= cap; kk <<= 1) {
        for (uint64_t j = kk >> 1; j >= (uint64_t)SORT_LOCAL; j >>= 1) {
            const uint64_t pairs = cap >> 1;
            const int g = (int)((pairs / 256) < 16384 ? (pairs / 256) : 16384);
            hipLaunchKernelGGL((k_bitonic_global<P>), dim3(g), dim3(256), 0, s, ok, opos, cap, j, kk);
        }
        hipLaunchKernelGGL((k_bitonic_local<P>), dim3(lgrid), dim3(1024), 0, s, ok, opos, kk, kk);
    }
}
}  // namespace

hipError_t launch_exact_sort(hipStream_t s, const double* scores, uint64_t n, uint64_t k, uint64_t* okeys,
                             uint32_t* opos, uint32_t* out_pos, double* out_scores)
{
    if (n == 0 || n >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t cap = sort_capacity_for(n);
    unsigned long long* ok = reinterpret_cast<unsigned long long*>(okeys);
    const int tgrid = (int)((cap / 256) < 8192 ? (cap / 256) : 8192);
    hipLaunchKernelGGL(k_sort_init, dim3(tgrid), dim3(256), 0, s, scores, n, cap, ok, opos);
    bitonic_network<uint32_t>(s, ok, opos, cap);
    const uint64_t kk = k < n ? k : n;
    if (kk > 0) {
        const int egrid = (int)(((kk + 255) / 256) < 4096 ? ((kk + 255) / 256) : 4096);
        hipLaunchKernelGGL(k_sort_emit, dim3(egrid), dim3(256), 0, s, opos, scores, kk, out_pos, out_scores);
    }
    return hipGetLastError();
}

hipError_t launch_hnsw_distances(hipStream_t s, int metric, const double* master, const double* q64,
                                 uint32_t dim, const uint32_t* positions, uint32_t m, uint64_t* out)
{
    if (m == 0) return hipSuccess;
    const int grid = (int)((m + KP - 1) / KP);
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_hnsw_dist<MM>), dim3(grid), dim3(256), 0, s, master, q64, dim, positions, m,
                           reinterpret_cast<unsigned long long*>(out));
        return hipGetLastError();
    });
}

// ---- range search -------------------------------------------------------------------------------
// The range scan's shapes are the subset scan's: for every stride VL_SCAN_VARIANTS specialises, k_scan's default entry.
bool scan_range_takes_qarg(uint32_t ld) { return scan_takes_qarg(ld); }

hipError_t launch_scan_range(hipStream_t s, int metric, const float* slab, const float* inv_norm, const uint32_t* plist,
                             uint64_t n, const double* q64, uint32_t dim, uint32_t ld, float tau, uint32_t* cand,
                             uint32_t cap, uint32_t* ctr, ScanPlan* plan, const float* q32_host)
{
    if (n == 0 || n >= 0xFFFFFFFFull || (ld & 3) || cap == 0) return hipErrorInvalidValue;
    const ScanShape sh = default_scan_shape(ld / 4);
    const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
    if (!shape_takes_qarg(sh, ld, q32_host) && !q64) return hipErrorInvalidValue;
    int grid = 0;
    hipError_t rc = dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        const auto head = std::make_tuple(slab4, inv_norm, plist);
        const auto tail = std::make_tuple(tau, cand, cap, ctr);
        if (plist) return launch_scan_family<RangeFamily<MM, true>>(s, sh, n, ld, q64, dim, q32_host, head, tail, &grid);
        return launch_scan_family<RangeFamily<MM, false>>(s, sh, n, ld, q64, dim, q32_host, head, tail, &grid);
    });
    if (plan) {
        plan->grid = grid;
        plan->variant = sh.special ? (RANGE_VARIANT_BASE + sh.g * 10000 + sh.vpl * 100 + sh.u) : -(RANGE_VARIANT_BASE + sh.g);
    }
    return rc;
}

// ---- grouped search, pass 1: the range scan's shapes, GroupBestSink in RangeSink's place ------------------------------
hipError_t launch_scan_group_best(hipStream_t s, int metric, const float* slab, const float* inv_norm, const uint32_t* plist,
                                  uint64_t n, const double* q64, uint32_t dim, uint32_t ld, const uint32_t* group_of_row,
                                  uint64_t* best, ScanPlan* plan, const float* q32_host)
{
    if (n == 0 || n >= 0xFFFFFFFFull || (ld & 3) || !group_of_row || !best) return hipErrorInvalidValue;
    const ScanShape sh = default_scan_shape(ld / 4);
    const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
    if (!shape_takes_qarg(sh, ld, q32_host) && !q64) return hipErrorInvalidValue;
    int grid = 0;
    hipError_t rc = dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        const auto head = std::make_tuple(slab4, inv_norm, plist);
        const auto tail = std::make_tuple(group_of_row, reinterpret_cast<unsigned long long*>(best));
        if (plist) return launch_scan_family<GroupBestFamily<MM, true>>(s, sh, n, ld, q64, dim, q32_host, head, tail, &grid);
        return launch_scan_family<GroupBestFamily<MM, false>>(s, sh, n, ld, q64, dim, q32_host, head, tail, &grid);
    });
    if (plan) {
        plan->grid = grid;
        plan->variant = sh.special ? (GROUP_VARIANT_BASE + sh.g * 10000 + sh.vpl * 100 + sh.u) : -(GROUP_VARIANT_BASE + sh.g);
    }
    return rc;
}

hipError_t launch_range_rescore(hipStream_t s, int metric, const double* master, const double* q64, const uint32_t* cand,
                                uint32_t cap, uint32_t dim, double* scores, uint32_t* ctr)
{
    if (cap == 0) return hipErrorInvalidValue;
    // the candidate count is the device's: enough workgroups for a full buffer, those without a tile leave at once
    const uint32_t tiles = (cap + EX_ROWS - 1) / EX_ROWS;
    const int grid = (int)(tiles < 1024u ? tiles : 1024u);
    return dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_range_rescore<MM>), dim3(grid), dim3(256), 0, s, master, q64, cand, cap, dim, scores, ctr);
        return hipGetLastError();
    });
}

hipError_t launch_range_cut(hipStream_t s, const double* scores, const uint32_t* cand, const uint32_t* m_ptr, uint64_t m_max,
                            double min_score, uint64_t* keys, uint64_t* pv, uint64_t store_cap, uint32_t* ctr,
                            const uint32_t* group_of_row, uint64_t n_rows, bool keep_nan)
{
    if (m_max == 0 || m_max >= 0xFFFFFFFFull || store_cap >= 0xFFFFFFFFull || n_rows >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t blocks = (m_max + 255) / 256;
    const int grid = (int)(blocks < 2048 ? blocks : 2048);
    unsigned long long* k64 = reinterpret_cast<unsigned long long*>(keys);
    unsigned long long* p64 = reinterpret_cast<unsigned long long*>(pv);
    if (group_of_row)
        hipLaunchKernelGGL(k_range_cut<true>, dim3(grid), dim3(256), 0, s, scores, cand, m_ptr, (uint32_t)m_max, (uint32_t)m_max,
                           min_score, k64, p64, (uint32_t)store_cap, ctr, group_of_row, (uint32_t)n_rows, keep_nan ? 1 : 0);
    else
        hipLaunchKernelGGL(k_range_cut<false>, dim3(grid), dim3(256), 0, s, scores, cand, m_ptr, (uint32_t)m_max, (uint32_t)m_max,
                           min_score, k64, p64, (uint32_t)store_cap, ctr, (const uint32_t*)nullptr, 0u, 0);
    return hipGetLastError();
}

hipError_t launch_range_rank(hipStream_t s, uint64_t* keys, uint64_t* pv, const double* scores, const uint32_t* total_ptr,
                             uint64_t total, uint64_t k, uint32_t* out_pos, double* out_scores)
{
    unsigned long long* ok = reinterpret_cast<unsigned long long*>(keys);
    unsigned long long* op = reinterpret_cast<unsigned long long*>(pv);
    const uint64_t cap = total_ptr ? (uint64_t)RANGE_SMALL : sort_capacity_for(total);
    if (total_ptr && k > cap) k = cap;
    if (!total_ptr && (total == 0 || total >= 0xFFFFFFFFull)) return hipErrorInvalidValue;
    const int pgrid = (int)((cap / 256) < 4096 ? (cap / 256) : 4096);
    hipLaunchKernelGGL(k_range_pad, dim3(pgrid), dim3(256), 0, s, ok, op, total_ptr, total, cap);
    bitonic_network<unsigned long long>(s, ok, op, cap);
    if (k > 0) {
        const int egrid = (int)(((k + 255) / 256) < 4096 ? ((k + 255) / 256) : 4096);
        hipLaunchKernelGGL(k_range_emit, dim3(egrid), dim3(256), 0, s, op, scores, total_ptr, k, out_pos, out_scores);
    }
    return hipGetLastError();
}

hipError_t launch_range_batch_tail(hipStream_t s, int metric, const Cand32* cand, const uint32_t* cnt, uint32_t cap, uint32_t nq,
                                   const double* master, const double* q64, const double* min_scores, uint32_t dim,
                                   uint64_t n_rows, uint32_t emit_cap, double* sv_score, uint32_t* sv_pos, uint32_t* ctr,
                                   uint32_t* out_pos, double* out_scores)
{
    if (nq == 0 || cap == 0 || n_rows == 0 || n_rows >= 0xFFFFFFFFull || emit_cap > RBATCH_SEG) return hipErrorInvalidValue;
    // 8 workgroups share a query's tiles of 16 candidates (tens of candidates: 2-3 tiles; a full buffer: 32 tiles each)
    const hipError_t rc = dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        hipLaunchKernelGGL((k_rbatch_rescore_cut<MM>), dim3(8, nq), dim3(256), 0, s, cand, cnt, cap, master, q64, min_scores, dim,
                           (uint32_t)n_rows, sv_score, sv_pos, ctr);
        return hipGetLastError();
    });
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(k_rbatch_offsets, dim3(1), dim3(256), 0, s, cnt, cap, nq, emit_cap, ctr);
    if (emit_cap > 0) hipLaunchKernelGGL(k_rbatch_rank_emit, dim3(nq), dim3(256), 0, s, sv_score, sv_pos, ctr, out_pos, out_scores);
    return hipGetLastError();
}

}  // namespace vl
