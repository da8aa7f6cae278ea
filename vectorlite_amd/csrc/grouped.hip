// grouped.hip -- grouped search (best row per group): everything except the two slab scans, which
// are scan_stream() instantiations in kernels.hip.
//   k_group_rows       the group table's resolution: storage position -> dense group number
//   k_group_top(_final) the 64 largest values of pass 1's best[] (TopList / block_merge / the list merge), decoded
//   k_group_first, k_group_collapse   the collapse of the ranked survivors to one row per group
//   k_group_keep_bits  the keep bitmap of S for the batched form (section 26)
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "group_plan.hpp"
#include "kernels.hpp"

namespace vl {
namespace {
using namespace dev;

// group_of_row[p] = dense[i] when pos_ids[p] == fids[i] (fids sorted, unique: the filter resolution's lower bound), else GROUP_NONE
__global__ __launch_bounds__(256) void k_group_rows(const unsigned long long* __restrict__ pos_ids, uint32_t n,
                                                    const unsigned long long* __restrict__ fids,
                                                    const uint32_t* __restrict__ dense, uint32_t nf,
                                                    uint32_t* __restrict__ group_of_row)
{
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const unsigned long long id = pos_ids[p];
        uint32_t lo = 0, hi = nf;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (fids[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        group_of_row[p] = (lo < nf && fids[lo] == id) ? dense[lo] : GROUP_NONE;
    }
}

// A slot of best[] back to the scan's (key, position): 0 = no row of that group was scanned.
__device__ __forceinline__ float ordered_to_key(uint32_t o)
{
    return __int_as_float((int)((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o));
}

// One pass over best[]: per-wave top-64 lists of the decoded (key, position) pairs -- the order of the u64 values, since
// the position breaks ties the same way -- merged per workgroup; list blockIdx.x of `lists`.
__global__ __launch_bounds__(1024) void k_group_top(const unsigned long long* __restrict__ best, uint32_t n_groups,
                                                    Cand32* __restrict__ lists)
{
    __shared__ Cand32 sh[16 * WAVE];
    TopList<float> L;
    L.init();
    const uint32_t step = gridDim.x * 1024;
    for (uint32_t b0 = blockIdx.x * 1024; b0 < n_groups; b0 += step) {  // workgroup-uniform trip count
        const uint32_t g = b0 + threadIdx.x;
        const unsigned long long v = g < n_groups ? best[g] : 0ull;
        L.offer(ordered_to_key((uint32_t)(v >> 32)), 0xFFFFFFFFu - (uint32_t)v, v != 0ull);
    }
    block_merge<float, Cand32, 16>(L, sh);
    if ((threadIdx.x >> 6) == 0) {
        Cand32 e;
        e.key = L.key;
        e.pos = L.pos;
        lists[(size_t)blockIdx.x * KP + lane_id()] = e;
    }
}

// The n_lists <= 64 workgroup lists merged into one; its first min(k, entries) positions -> cand[], the count -> *count.
__global__ __launch_bounds__(1024) void k_group_top_final(const Cand32* __restrict__ lists, int n_lists, uint32_t k,
                                                          uint32_t* __restrict__ cand, uint32_t* __restrict__ count)
{
    __shared__ Cand32 sh[16 * WAVE];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    TopList<float> L;
    {
        const int first = wave * 4;
        int c = n_lists - first;
        c = c < 0 ? 0 : (c > 4 ? 4 : c);
        fold_lists4<float, Cand32>(L, lists, first, c);
    }
    block_merge<float, Cand32, 16>(L, sh);
    if (wave == 0) {
        const unsigned long long have = __ballot(L.pos != POS_SENTINEL);  // a prefix of the lanes: the list is sorted
        uint32_t c = (uint32_t)__popcll(have);
        if (c > k) c = k;
        if ((uint32_t)lane < c) cand[lane] = L.pos;
        if (lane == 0) *count = c;
    }
}

// first[g] = the rank of the first survivor of group g (first[] filled with 0xFF bytes by the caller)
__global__ __launch_bounds__(256) void k_group_first(const unsigned long long* __restrict__ pv, const uint32_t* __restrict__ n_ptr,
                                                     uint32_t n_val, uint32_t n_max, const uint32_t* __restrict__ group_of_row,
                                                     uint32_t n_rows, uint32_t n_groups, uint32_t* __restrict__ first)
{
    const uint32_t n = n_ptr ? *n_ptr : n_val;
    if (n > n_max) return;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t pos = (uint32_t)(pv[i] >> 32);
        if (pos >= n_rows) continue;
        const uint32_t g = group_of_row[pos];
        if (g < n_groups) atomicMin(first + g, i);
    }
}

// One workgroup walks the ranking in tiles of 1024: survivor i is kept iff first[group] == i, a prefix count over the tile
// gives its output slot, the walk ends once k are out.  Which survivor a group keeps does not depend on the order in which
// k_group_first's atomics landed, so the answer is deterministic.
__global__ __launch_bounds__(1024) void k_group_collapse(const unsigned long long* __restrict__ pv, const double* __restrict__ scores,
                                                         const uint32_t* __restrict__ n_ptr, uint32_t n_val, uint32_t n_max,
                                                         const uint32_t* __restrict__ group_of_row, uint32_t n_rows,
                                                         const unsigned long long* __restrict__ group_keys, uint32_t n_groups,
                                                         const uint32_t* __restrict__ first, uint32_t k,
                                                         unsigned long long* __restrict__ out_keys, uint32_t* __restrict__ out_pos,
                                                         double* __restrict__ out_scores, uint32_t* __restrict__ out_n)
{
    __shared__ uint32_t sh_cnt[16];
    const uint32_t n = n_ptr ? *n_ptr : n_val;
    if (n > n_max) return;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t base = 0;  // workgroup-uniform: survivors kept so far
    for (uint32_t t0 = 0; t0 < n && base < k; t0 += 1024) {
        const uint32_t i = t0 + threadIdx.x;
        unsigned long long e = 0;
        uint32_t g = GROUP_NONE;
        if (i < n) {
            e = pv[i];
            const uint32_t pos = (uint32_t)(e >> 32);
            if (pos < n_rows) g = group_of_row[pos];
        }
        const bool keep = g < n_groups && first[g] == i;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) sh_cnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            const uint32_t c = sh_cnt[w];
            if (w < wave) before += c;
            total += c;
        }
        const uint32_t slot = base + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (keep && slot < k) {
            out_keys[slot] = group_keys[g];
            out_pos[slot] = (uint32_t)(e >> 32);
            out_scores[slot] = scores[(uint32_t)e];
        }
        base += total;
        __syncthreads();  // sh_cnt is rewritten by the next tile
    }
    if (threadIdx.x == 0) *out_n = base < k ? base : k;
}

// The keep bitmap of S for the batched grouped search, in k_filter_bits' layout: one wave per 64-bit
// word, lane p & 63 tests p < n && group_of_row[p] != GROUP_NONE and, with a filter, the filter -- an exclusion token's own
// keep word (filter_keep), or membership of the row's id in an include token's sorted ids (fids; the lower bound of
// k_filter_bits' id_in_set).  Lane 0 stores the ballot (bits at or past n are 0) and adds its popcount to *m_out.
__global__ __launch_bounds__(256) void k_group_keep_bits(const uint32_t* __restrict__ group_of_row, uint32_t n,
                                                         const unsigned long long* __restrict__ filter_keep,
                                                         const unsigned long long* __restrict__ pos_ids,
                                                         const unsigned long long* __restrict__ fids, uint32_t nf, uint32_t by_ids,
                                                         uint32_t n_words, unsigned long long* __restrict__ keep,
                                                         uint32_t* __restrict__ m_out)
{
    const int lane = lane_id();
    const uint32_t n_waves = gridDim.x * 4;
    uint32_t mine = 0;  // lane 0: bits set in this wave's words
    for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < n_words; w += n_waves) {  // wave-uniform trip count
        const uint32_t p = w * 64u + (uint32_t)lane;
        bool on = p < n && group_of_row[p] != GROUP_NONE;
        if (filter_keep) {
            on = on && ((filter_keep[w] >> lane) & 1ull) != 0ull;
        } else if (by_ids && on) {
            const unsigned long long id = pos_ids[p];
            uint32_t lo = 0, hi = nf;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (fids[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            on = lo < nf && fids[lo] == id;
        }
        const unsigned long long word = __ballot(on);
        if (lane == 0) {
            keep[w] = word;
            mine += (uint32_t)__popcll(word);
        }
    }
    if (lane == 0 && mine) atomicAdd(m_out, mine);
}

}  // namespace

hipError_t launch_group_keep_bits(hipStream_t s, const uint32_t* group_of_row, uint64_t n, const unsigned long long* filter_keep,
                                  const unsigned long long* pos_ids, const unsigned long long* fids, uint64_t nf,
                                  unsigned long long* keep, uint32_t* m_out)
{
    const bool by_ids = !filter_keep && pos_ids != nullptr;  // an include token (nf == 0: it keeps no row, fids is not read)
    if (n == 0 || n >= 0xFFFFFFFFull || nf >= 0xFFFFFFFFull || !group_of_row || !keep || !m_out || (by_ids && nf != 0 && !fids))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(m_out, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint64_t n_words = (n + 63) / 64;
    const uint64_t blocks = (n_words + 3) / 4;
    const int grid = (int)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(k_group_keep_bits, dim3(grid), dim3(256), 0, s, group_of_row, (uint32_t)n, filter_keep, pos_ids, fids,
                       (uint32_t)nf, by_ids ? 1u : 0u, (uint32_t)n_words, keep, m_out);
    return hipGetLastError();
}

hipError_t launch_group_rows(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                             const uint32_t* dense, uint64_t nf, uint32_t* group_of_row)
{
    if (n == 0 || n >= 0xFFFFFFFFull || nf == 0 || nf >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t blocks = (n + 255) / 256;
    const int grid = (int)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(k_group_rows, dim3(grid), dim3(256), 0, s, pos_ids, (uint32_t)n, fids, dense, (uint32_t)nf, group_of_row);
    return hipGetLastError();
}

hipError_t launch_group_top(hipStream_t s, const uint64_t* best, uint64_t n_groups, uint32_t k, Cand32* lists, uint32_t* cand,
                            uint32_t* ctr)
{
    if (n_groups == 0 || n_groups >= 0xFFFFFFFFull || k == 0 || k > (uint32_t)KP) return hipErrorInvalidValue;
    const uint64_t blocks = (n_groups + 1023) / 1024;
    const int grid = (int)(blocks < (uint64_t)GROUP_TOP_LISTS ? blocks : (uint64_t)GROUP_TOP_LISTS);
    hipLaunchKernelGGL(k_group_top, dim3(grid), dim3(1024), 0, s, reinterpret_cast<const unsigned long long*>(best),
                       (uint32_t)n_groups, lists);
    hipLaunchKernelGGL(k_group_top_final, dim3(1), dim3(1024), 0, s, (const Cand32*)lists, grid, k, cand, ctr + RANGE_CTR_APPENDED);
    return hipGetLastError();
}

hipError_t launch_group_collapse(hipStream_t s, const uint64_t* pv, const double* scores, const uint32_t* n_ptr, uint64_t n_max,
                                 const uint32_t* group_of_row, uint64_t n_rows, const uint64_t* group_keys, uint64_t n_groups,
                                 uint32_t* first, uint32_t k, uint64_t* out_keys, uint32_t* out_pos, double* out_scores,
                                 uint32_t* out_n)
{
    if (n_max == 0 || n_max >= 0xFFFFFFFFull || n_rows >= 0xFFFFFFFFull || n_groups == 0 || n_groups >= 0xFFFFFFFFull || k == 0 ||
        k > GROUPED_MAX_K)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(first, 0xFF, n_groups * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const unsigned long long* p64 = reinterpret_cast<const unsigned long long*>(pv);
    const uint64_t blocks = (n_max + 255) / 256;
    const int grid = (int)(blocks < 2048 ? blocks : 2048);
    hipLaunchKernelGGL(k_group_first, dim3(grid), dim3(256), 0, s, p64, n_ptr, (uint32_t)n_max, (uint32_t)n_max, group_of_row,
                       (uint32_t)n_rows, (uint32_t)n_groups, first);
    hipLaunchKernelGGL(k_group_collapse, dim3(1), dim3(1024), 0, s, p64, scores, n_ptr, (uint32_t)n_max, (uint32_t)n_max, group_of_row,
                       (uint32_t)n_rows, reinterpret_cast<const unsigned long long*>(group_keys), (uint32_t)n_groups,
                       (const uint32_t*)first, k, reinterpret_cast<unsigned long long*>(out_keys), out_pos, out_scores, out_n);
    return hipGetLastError();
}

}  // namespace vl
