// scan_stream.hpp -- the single-query streaming row scan, written once.
//
// Every single-query scan (k_scan, k_scan_subset, k_scan_range and their _q64 forms in kernels.hip; k_scan_bf16,
// k_scan_bf16_qarg and k_scan_i8_qarg in mfma_scan.hip) is scan_stream() below with three small policies:
//   * a ROW FORMAT (F32Rows, Bf16Rows, I8Rows: next to their arithmetic in the two .hip files): what a 16-byte chunk
//     is, which per-row scalars travel with the row loads, how a chunk meets the lane's query slice, how the reduced
//     sum becomes a key;
//   * a ROW SOURCE (AllRows, ListedRows, MaskedRows): which storage position step i scores, and whether it may be offered;
//   * a SINK (TopSink, RangeSink, GroupBestSink): what happens to (key, position, valid).
// The run-time-stride f32 kernels (k_scan_generic and its subset / range forms) share the sources and sinks through
// the much smaller scan_stream_generic() in kernels.hip.
#pragma once

#include "device_common.hpp"
#include "group_plan.hpp"

namespace vl {
namespace dev {

template <int G>
__device__ __forceinline__ float group_reduce(float a)
{
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) a += __shfl_xor(a, o);
    return a;
}

// The query arrives as f64 (the reference's `search(&[f64])`); each lane rounds its own slice to
// f32 (round to nearest even, the same rounding the slab rows got at ingest).  Columns past `dim`
// (slab padding) read as zero.
__device__ __forceinline__ f32x4 load_q4(const double* __restrict__ q64, uint32_t j4, uint32_t dim)
{
    // Clamped, never predicated: `i < dim ? q64[i] : 0` makes hipcc branch around every load and wait for
    // each in turn (48 dependent L2 round trips in the prologue of every wave of the dim-384 scan).
    const uint32_t i = j4 * 4, last = dim - 1;
    const double v0 = q64[i + 0 < dim ? i + 0 : last];
    const double v1 = q64[i + 1 < dim ? i + 1 : last];
    const double v2 = q64[i + 2 < dim ? i + 2 : last];
    const double v3 = q64[i + 3 < dim ? i + 3 : last];
    f32x4 r;
    r.x = i + 0 < dim ? (float)v0 : 0.0f;
    r.y = i + 1 < dim ? (float)v1 : 0.0f;
    r.z = i + 2 < dim ? (float)v2 : 0.0f;
    r.w = i + 3 < dim ? (float)v3 : 0.0f;
    return r;
}

// ---- row sources -------------------------------------------------------------------------------------------------
// at(i, n): the storage position of row i of the n rows to score; i == n marks "no row" (the tail of the last step).
// load_row(): the row whose bytes are loaded for it.  Loads are clamped into bounds and never predicated: a row that
// is not there is loaded from a row that is, and dropped at the sink.

// MASKED: the source drops rows at the sink (MaskedRows).  For the other sources it is a compile-time false and every
// line it guards is gone: their kernels are the code they were before the hook existed.

// Every row of the slab, in storage order.
struct AllRows {
    static constexpr bool INDIRECT = false, MASKED = false;
    __device__ __forceinline__ uint32_t at(uint32_t i, uint32_t) const { return i; }
    __device__ __forceinline__ uint32_t load_row(uint32_t pos, bool valid, uint32_t n) const { return valid ? pos : n - 1; }
};

// The rows plist[0..n): ascending storage positions (an id filter's resolution).  The position is one dependent read
// away from the row loads, so the scans request it one iteration ahead (INDIRECT).
struct ListedRows {
    static constexpr bool INDIRECT = true, MASKED = false;
    const uint32_t* __restrict__ plist;
    __device__ __forceinline__ uint32_t at(uint32_t i, uint32_t n) const { return plist[i < n ? i : n - 1]; }
    __device__ __forceinline__ uint32_t load_row(uint32_t pos, bool, uint32_t) const { return pos; }
};

// Every row of the slab like AllRows, minus the rows whose bit in `keep` is 0 (an exclusion filter's resolution: bit p & 63
// of word p >> 6 is set iff row p qualifies; bits at or past n are 0).  The rows are all loaded and scored -- an exclusion
// set leaves almost every row in play -- and an excluded one is dropped where it would be offered.  The WAVE / G rows of
// one wave step are consecutive and start at a multiple of WAVE / G, a divisor of 64: their keep bits are one shifted
// field of ONE aligned 64-bit word at a wave-uniform address, so the read is a scalar load (no VGPR per row group) that
// goes out together with the step's row loads.
struct MaskedRows {
    static constexpr bool INDIRECT = false, MASKED = true;
    const unsigned long long* __restrict__ keep;
    __device__ __forceinline__ uint32_t at(uint32_t i, uint32_t) const { return i; }
    __device__ __forceinline__ uint32_t load_row(uint32_t pos, bool valid, uint32_t n) const { return valid ? pos : n - 1; }
    // first_row: wave-uniform (the caller passes it through readfirstlane)
    __device__ __forceinline__ unsigned long long keep_word(uint32_t first_row) const { return keep[first_row >> 6]; }
};

// ---- sinks -------------------------------------------------------------------------------------------------------
// offer(u, key, pos, active): lane c == 0 of row group u of the iteration hands its row over (active: the row exists);
// step(): the iteration's U row groups are through; finish(): the stream is.

// Top-k: one sorted top-64 list per wave, the workgroup's four merged through LDS, written as list blockIdx.x of `out`.
// Positions reach offer() in ascending order within a wave's stream, so ties keep the lower position.
struct TopSink {
    Cand32* __restrict__ out;
    TopList<float> L;
    __device__ __forceinline__ explicit TopSink(Cand32* __restrict__ o) : out(o) { L.init(); }
    __device__ __forceinline__ void offer(int, float key, uint32_t pos, bool active) { L.offer(key, pos, active); }
    __device__ __forceinline__ void step() {}
    __device__ __forceinline__ void finish()
    {
        __shared__ Cand32 sh[4 * WAVE];
        block_merge<float, Cand32, 4>(L, sh);
        if ((threadIdx.x >> 6) == 0) {
            Cand32 e;
            e.key = L.key;
            e.pos = L.pos;
            out[(size_t)blockIdx.x * KP + lane_id()] = e;
        }
    }
};

// The wave ballots the U flags of an iteration, ONE lane reserves the slots of all of them with one global atomic add
// on *ctr, the flagged lanes store their positions.  The counter keeps counting past `cap`; stores past it are dropped.
template <int U>
__device__ __forceinline__ void range_append(const bool (&hit)[U], const uint32_t (&pos)[U], uint32_t* __restrict__ cand,
                                             uint32_t cap, uint32_t* __restrict__ ctr)
{
    const int lane = lane_id();
    unsigned long long bal[U];
    uint32_t total = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        bal[u] = __ballot(hit[u]);
        total += (uint32_t)__popcll(bal[u]);
    }
    if (total == 0) return;  // wave-uniform: a selective threshold leaves the stream alone
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(ctr, total);
    base = __shfl(base, 0);
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t slot = base + (uint32_t)__popcll(bal[u] & below);
        if (hit[u] && slot < cap) cand[slot] = pos[u];
        base += (uint32_t)__popcll(bal[u]);
    }
}

// Range search: the scan that APPENDS.  A row is a candidate unless key <= tau (tau: the
// largest key whose bound_for_key is below the caller's score threshold, chosen on the host; a NaN tau or key fails
// the comparison and keeps the row).  No LDS list, no block merge, no partial lists.
template <int U>
struct RangeSink {
    float tau;
    uint32_t* __restrict__ cand;
    uint32_t cap;
    uint32_t* __restrict__ ctr;
    bool hit[U];
    uint32_t at[U];
    __device__ __forceinline__ RangeSink(float t, uint32_t* __restrict__ cd, uint32_t cp, uint32_t* __restrict__ ct)
        : tau(t), cand(cd), cap(cp), ctr(ct)
    {
    }
    __device__ __forceinline__ void offer(int u, float key, uint32_t pos, bool active)
    {
        hit[u] = active && !(key <= tau);
        at[u] = pos;
    }
    __device__ __forceinline__ void step() { range_append<U>(hit, at, cand, cap, ctr); }
    __device__ __forceinline__ void finish() {}
};

// Grouped search, pass 1: the scan that keeps the best key PER GROUP.  A row of group g raises
// best[g] to (ordered bits of its key) << 32 | (0xFFFFFFFF - position): larger key first, lower position on ties, never 0
// for a row that is there (best[] is zeroed in front of the launch).  A load goes in front of the atomic and the lane
// skips the atomic when its value would not raise the slot: values only grow, so a stale read costs an atomic and never
// loses a row.  The U group numbers of an iteration are requested together, then the U slots.  No LDS, no block merge.
__device__ __forceinline__ uint32_t key_to_ordered(float key)
{
    const uint32_t b = (uint32_t)__float_as_int(key);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <int U>
struct GroupBestSink {
    const uint32_t* __restrict__ group_of_row;
    unsigned long long* __restrict__ best;
    bool on[U];
    unsigned long long val[U];
    __device__ __forceinline__ GroupBestSink(const uint32_t* __restrict__ gor, unsigned long long* __restrict__ b)
        : group_of_row(gor), best(b)
    {
    }
    __device__ __forceinline__ void offer(int u, float key, uint32_t pos, bool active)
    {
        on[u] = active;
        val[u] = ((unsigned long long)key_to_ordered(key) << 32) | (unsigned long long)(0xFFFFFFFFu - pos);
    }
    __device__ __forceinline__ void step()
    {
        uint32_t g[U];
        unsigned long long seen[U];
#pragma unroll
        for (int u = 0; u < U; ++u) g[u] = on[u] ? group_of_row[0xFFFFFFFFu - (uint32_t)val[u]] : GROUP_NONE;
#pragma unroll
        for (int u = 0; u < U; ++u)
            seen[u] = g[u] != GROUP_NONE ? __hip_atomic_load(best + g[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (seen[u] < val[u]) (void)__hip_atomic_fetch_max(best + g[u], val[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void finish() {}
};

// ---- the loop ----------------------------------------------------------------------------------------------------
// A row is Fmt::VPL * G chunks of 16 bytes; the G lanes of a row group share a row (lane c holds chunks c + G j and
// the matching slice `qv` of the query, loaded by the kernel entry), a wave scores WAVE / G rows per step and keeps U
// steps in flight.  Waves of the grid stride over the steps.  A format provides
//   Chunk, Query, Scalars, VPL, slab
//   load_scalars(r)           the per-row scalars, requested TOGETHER WITH the row loads, not after them
//   accumulate(a, chunk, q)   one chunk against the lane's query slice
//   key(sum, scalars)         larger = better
// The policies are taken BY VALUE: through references hipcc must assume that the sink's list and the other policies
// alias, carries copies around the loop and spends two to four more VGPRs (an occupancy step at 64 and 84).
template <int G, int U, class Fmt, class Rows, class Sink>
__device__ __forceinline__ void scan_stream(const Fmt fmt, const typename Fmt::Query (&qv)[Fmt::VPL], const Rows rows,
                                            uint32_t n, Sink sink)
{
    constexpr int VPL = Fmt::VPL;
    constexpr int RPS = WAVE / G;  // rows per step of one wave
    constexpr uint32_t LDC = G * VPL;

    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int g = lane / G, c = lane % G;

    const uint32_t n_steps = (n + RPS - 1) / RPS;
    const uint32_t n_waves = gridDim.x * 4;
    const uint32_t wave_global = blockIdx.x * 4 + wave;
    const uint32_t stride = n_waves * U;

    auto fetch = [&](uint32_t s0, uint32_t (&pos)[U], bool (&valid)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t s = s0 + (uint32_t)u * n_waves;
            const uint32_t i = s < n_steps ? s * RPS + g : n;  // n marks "no row"
            valid[u] = i < n;
            pos[u] = rows.at(i, n);
        }
    };
    uint32_t pos_next[U];
    bool valid_next[U];
    if constexpr (Rows::INDIRECT) fetch(wave_global, pos_next, valid_next);

    for (uint32_t s0 = wave_global; s0 < n_steps; s0 += stride) {
        uint32_t pos[U];
        bool valid[U];
        if constexpr (Rows::INDIRECT) {
            // the list entries of the NEXT iteration are requested before this iteration's row loads, so that read is
            // in flight while the rows stream and never stands alone in front of them
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pos[u] = pos_next[u];
                valid[u] = valid_next[u];
            }
            fetch(s0 + stride, pos_next, valid_next);
            __builtin_amdgcn_sched_barrier(0);  // the list loads go out in front of the row loads
        } else {
            fetch(s0, pos, valid);
        }
        typename Fmt::Chunk x[U][VPL];
        typename Fmt::Scalars sc[U];
        [[maybe_unused]] unsigned long long kw[U];  // MaskedRows: the keep word of each step in flight
        [[maybe_unused]] uint32_t first[U];         // and the step's first row (wave-uniform)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t r = rows.load_row(pos[u], valid[u], n);
            const typename Fmt::Chunk* p = fmt.slab + (size_t)r * LDC + c;
#pragma unroll
            for (int j = 0; j < VPL; ++j) x[u][j] = __builtin_nontemporal_load(p + G * j);
            sc[u] = fmt.load_scalars(r);
            if constexpr (Rows::MASKED) {
                // s0 is the same in every lane of the wave; readfirstlane tells the compiler so
                const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s0) + (uint32_t)u * n_waves;
                first[u] = s < n_steps ? s * RPS : 0u;  // a step past the end reads word 0 and offers nothing
                kw[u] = rows.keep_word(first[u]);
            }
        }
        // every load of this iteration is issued before the first arithmetic instruction: left alone, the scheduler
        // trades memory-level parallelism for registers and serialises the loads two at a time
        __builtin_amdgcn_sched_barrier(0);
        [[maybe_unused]] unsigned long long kept[U];
        if constexpr (Rows::MASKED) {
            // The step's RPS keep bits, spread to the wave's lanes with scalar instructions only: bit r of the field goes
            // to lane r * G, the lane that offers row r.  The lane mask waits for the offer in scalar registers and becomes
            // the lanes' flag there (inverse ballot): no VGPR, neither across the loop nor on top of the arithmetic's peak.
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned long long field = kw[u] >> (first[u] & 63u);  // wave-uniform: a scalar shift
                unsigned long long m = 0;
#pragma unroll
                for (int r = 0; r < RPS; ++r) m |= ((field >> r) & 1ull) << (r * G);
                kept[u] = m;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float a = 0.0f;
#pragma unroll
            for (int j = 0; j < VPL; ++j) a = Fmt::accumulate(a, x[u][j], qv[j]);
            a = group_reduce<G>(a);
            bool keep = true;
            if constexpr (Rows::MASKED) keep = __builtin_amdgcn_inverse_ballot_w64(kept[u]);
            sink.offer(u, fmt.key(a, sc[u]), pos[u], valid[u] && keep && c == 0);
        }
        sink.step();
    }
    sink.finish();
}

}  // namespace dev
}  // namespace vl
