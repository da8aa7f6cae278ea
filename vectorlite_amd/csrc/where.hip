// where.hip -- attribute columns and predicate filter tokens resolved on the device.
//   k_attr_rows      a column's resolution: storage position -> int64 value, and the "has a value" bitmap
//   k_where_bits     a predicate's resolution: the keep bitmap and the per-chunk kept-row counts, in one pass over the columns
//   k_where_compact  the ascending position list from the keep bitmap and the chunk offsets
// The counts become offsets (and m) through k_filter_scan (kernels.hip, launch_filter_scan).
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "kernels.hpp"
#include "where_plan.hpp"

namespace vl {
static_assert(WHERE_COUNTS_MAX == (uint32_t)FILTER_COUNTS_MAX, "the predicate path's counts go through k_filter_scan");
namespace {
using namespace dev;

// One wave per 64-bit word of the has-bitmap (k_filter_bits' layout).  Lane p & 63 takes the lower bound of its row's id over
// the column's sorted ids (k_group_rows' search): value_of_row[p] = the id's value, or 0 where the column does not hold the
// id.  Lane 0 stores the ballot of "holds it" (bits at or past n are 0) and adds its popcount to *rows_out.
__global__ __launch_bounds__(256) void k_attr_rows(const unsigned long long* __restrict__ pos_ids, uint32_t n,
                                                   const unsigned long long* __restrict__ fids, const long long* __restrict__ fvals,
                                                   uint32_t nf, uint32_t n_words, long long* __restrict__ value_of_row,
                                                   unsigned long long* __restrict__ has, uint32_t* __restrict__ rows_out)
{
    const int lane = lane_id();
    const uint32_t n_waves = gridDim.x * 4;
    uint32_t mine = 0;  // lane 0: bits set in this wave's words
    for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < n_words; w += n_waves) {  // wave-uniform trip count
        const uint32_t p = w * 64u + (uint32_t)lane;
        bool on = false;
        if (p < n) {
            const unsigned long long id = pos_ids[p];
            uint32_t lo = 0, hi = nf;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (fids[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            on = lo < nf && fids[lo] == id;
            value_of_row[p] = on ? fvals[lo] : 0ll;
        }
        const unsigned long long word = __ballot(on);
        if (lane == 0) {
            has[w] = word;
            mine += (uint32_t)__popcll(word);
        }
    }
    if (lane == 0 && mine) atomicAdd(rows_out, mine);
}

// Workgroup b owns the positions [b chunk, (b + 1) chunk), chunk a multiple of 64 (where_grid_for): whole keep words.  One
// wave per word: lane p & 63 loads its row's value of each clause's column (the wave reads 512 contiguous bytes per column
// and word) and its bit of the column's has-word, evaluates the conjunction and ballots; lane 0 stores the word with an
// ordinary store.  A row past n is never loaded and never kept, so the tail word's bits at or past n are 0 whatever
// value_of_row holds there.  counts[b] = the rows the chunk keeps.
__global__ __launch_bounds__(256) void k_where_bits(uint32_t n, uint32_t n_words, uint32_t chunk_words, WhereClausesDev c,
                                                    unsigned long long* __restrict__ keep, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t sh_cnt[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t w_lo = blockIdx.x * chunk_words;
    const uint32_t w_hi = (uint64_t)w_lo + chunk_words < n_words ? w_lo + chunk_words : n_words;
    uint32_t cnt = 0;  // the same in every lane of the wave
    for (uint32_t w = w_lo + (uint32_t)wave; w < w_hi; w += 4) {  // wave-uniform trip count
        const uint32_t p = w * 64u + (uint32_t)lane;
        bool on = p < n;
#pragma unroll
        for (uint32_t i = 0; i < WHERE_MAX_CLAUSES; ++i) {
            if (i < c.n_clauses) {
                const bool has = ((c.has[i][w] >> lane) & 1ull) != 0ull;
                const long long v = p < n ? c.value_of_row[i][p] : 0ll;
                on = on && has && ((c.lo[i] <= v && v <= c.hi[i]) != (c.negate[i] != 0u));
            }
        }
        const unsigned long long word = __ballot(on);
        if (lane == 0) keep[w] = word;
        cnt += (uint32_t)__popcll(word);
    }
    if (lane == 0) sh_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
}

// The kept positions of chunk b, ascending, at offsets[b]: tiles of four keep words (256 positions), a wave per word;
// k_filter_compact's ranking with the keep bit in the place of the id lookup.
__global__ __launch_bounds__(256) void k_where_compact(const unsigned long long* __restrict__ keep, uint32_t n_words,
                                                       uint32_t chunk_words, const uint32_t* __restrict__ offsets, uint32_t m_cap,
                                                       uint32_t* __restrict__ plist)
{
    __shared__ uint32_t sh_cnt[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t w_lo = blockIdx.x * chunk_words;
    const uint32_t w_hi = (uint64_t)w_lo + chunk_words < n_words ? w_lo + chunk_words : n_words;
    uint32_t base = offsets[blockIdx.x];
    for (uint32_t w0 = w_lo; w0 < w_hi; w0 += 4) {  // block-uniform trip count
        const uint32_t w = w0 + (uint32_t)wave;
        const unsigned long long word = w < w_hi ? keep[w] : 0ull;
        if (lane == 0) sh_cnt[wave] = (uint32_t)__popcll(word);
        __syncthreads();
        uint32_t before = 0;
        for (int v = 0; v < wave; ++v) before += sh_cnt[v];
        const uint32_t total = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
        const uint32_t rank = before + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
        if (((word >> lane) & 1ull) != 0ull && base + rank < m_cap) plist[base + rank] = w * 64u + (uint32_t)lane;
        base += total;
        __syncthreads();  // sh_cnt is rewritten by the next tile
    }
}

}  // namespace

hipError_t launch_attr_rows(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                            const long long* fvals, uint64_t nf, long long* value_of_row, unsigned long long* has, uint32_t* rows_out)
{
    if (n == 0 || n >= 0xFFFFFFFFull || nf >= 0xFFFFFFFFull || !pos_ids || !value_of_row || !has || !rows_out ||
        (nf != 0 && (!fids || !fvals)))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(rows_out, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint64_t n_words = (n + 63) / 64;
    const uint64_t blocks = (n_words + 3) / 4;
    const int grid = (int)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(k_attr_rows, dim3(grid), dim3(256), 0, s, pos_ids, (uint32_t)n, fids, fvals, (uint32_t)nf, (uint32_t)n_words,
                       value_of_row, has, rows_out);
    return hipGetLastError();
}

hipError_t launch_where_bits(hipStream_t s, uint64_t n, const WhereClausesDev& clauses, unsigned long long* keep, uint32_t* counts,
                             uint32_t* m_out)
{
    if (n == 0 || n >= 0xFFFFFFFFull || clauses.n_clauses == 0 || clauses.n_clauses > WHERE_MAX_CLAUSES || !keep || !counts || !m_out)
        return hipErrorInvalidValue;
    for (uint32_t i = 0; i < clauses.n_clauses; ++i)
        if (!clauses.value_of_row[i] || !clauses.has[i]) return hipErrorInvalidValue;
    uint32_t chunk = 0;
    const uint32_t grid = where_grid_for(n, &chunk);
    hipLaunchKernelGGL(k_where_bits, dim3(grid), dim3(256), 0, s, (uint32_t)n, (uint32_t)((n + 63) / 64), chunk / 64, clauses, keep, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_filter_scan(s, counts, grid, m_out);
}

hipError_t launch_where_compact(hipStream_t s, uint64_t n, const unsigned long long* keep, const uint32_t* offsets, uint64_t m,
                                uint32_t* plist)
{
    if (n == 0 || n >= 0xFFFFFFFFull || m == 0 || m > n || !keep || !offsets || !plist) return hipErrorInvalidValue;
    uint32_t chunk = 0;
    const uint32_t grid = where_grid_for(n, &chunk);
    hipLaunchKernelGGL(k_where_compact, dim3(grid), dim3(256), 0, s, keep, (uint32_t)((n + 63) / 64), chunk / 64, offsets, (uint32_t)m,
                       plist);
    return hipGetLastError();
}

}  // namespace vl
