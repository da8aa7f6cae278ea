// where_plan.hpp -- the host arithmetic of predicate filter tokens (vl_index_filter_create_where).
// No device code: tests/native/where_plan_test.cpp checks the properties below on the CPU.
//
// 1. The chunking of a predicate resolution.  The bits-and-count pass counts kept rows by whole 64-bit keep words, so a
//    workgroup's chunk of positions must be a multiple of 64 -- which the id resolution's chunk (ceil(n / 1024) rows once
//    n > 1 048 576) is not.  where_grid_for gives the predicate path its own: the same rule rounded up to 64, used by the
//    count and by the compaction alike.
//      C1  the chunk is a multiple of 64 and at least 1024
//      C2  grid * chunk >= n > (grid - 1) * chunk, and 1 <= grid <= WHERE_COUNTS_MAX for 1 <= n < 2^32 - 1
//
// 2. The route of a single search under a predicate token: the position list with k_scan_subset, or the masked
//    int8 -> bf16 -> f32 ladder (section 23).  An exclusion token keeps almost every row and always takes the ladder; a
//    predicate may keep 0.01 % of the rows or 99 %.  Both routes are bound by the bytes they stream:
//      list    m * ld * 4            k_scan_subset reads the f32 rows of the kept positions
//      ladder  len * (row bytes of the FIRST stage the ladder would run for this handle and query: ldb for the int8
//              copy, 2 * ldb for the bf16 copy, 4 * ld for the f32 slab)
//    so the crossover sits near 25 % kept when int8 is the first stage, near 50 % under bf16, and the list always wins
//    when f32 is the first stage.  The rule is DERIVED from these byte counts; it agrees with the recorded pairs at
//    10 M x 384 (10 % kept: 0.279 ms through the list against 0.62 ms masked; 50 % kept: 1.17 ms against 0.617 ms) but has
//    not been measured for itself (tools/where_probe.py is there to do that).
//      W1  mode "list" never takes the ladder; an input that is not eligible never takes it in any mode
//      W2  mode "mask" takes it whenever the input is eligible
//      W3  mode "auto" takes it iff it is eligible and the ladder's estimate is strictly below the list's
//      W4  under "auto" the decision is monotone in m: once the ladder is taken it is taken for every larger m
//      W5  under "auto" the ladder is never taken when f32 is its first stage (ld * 4 * len >= ld * 4 * m)
//      W6  the decision is a function of its arguments
#pragma once

#include <stdint.h>

#include <algorithm>

namespace vl {

constexpr uint32_t WHERE_COUNTS_MAX = 1024;  // chunks of one resolution (FILTER_COUNTS_MAX: they share k_filter_scan)
constexpr uint32_t WHERE_MAX_CLAUSES = 4;

inline uint32_t where_grid_for(uint64_t n, uint32_t* chunk)
{
    uint64_t c = (n + WHERE_COUNTS_MAX - 1) / WHERE_COUNTS_MAX;
    if (c < 1024) c = 1024;
    c = (c + 63) / 64 * 64;
    *chunk = (uint32_t)c;
    return (uint32_t)((n + c - 1) / c);
}

enum : int { WHERE_ROUTE_AUTO = 0, WHERE_ROUTE_LIST = 1, WHERE_ROUTE_MASK = 2 };
enum : int { WHERE_STAGE_I8 = 0, WHERE_STAGE_BF16 = 1, WHERE_STAGE_F32 = 2 };

struct WhereShape {
    bool ladder_ok;   // no forced path, no out-of-domain row, the masked f32 scan is compiled for the stride
    uint64_t len;     // rows of the index
    uint32_t ld;      // f32 row stride, in values
    uint32_t ldb;     // row stride of the bf16 and int8 copies, in values
    int first_stage;  // WHERE_STAGE_*: what the ladder would run first for this handle and query
    uint64_t k_max;   // KFAST_MAX: the 64-entry list must keep a margin
};

inline bool where_mask_eligible(const WhereShape& s, uint64_t m, uint64_t k)
{
    return s.ladder_ok && m > 0 && std::min<uint64_t>(k, m) <= s.k_max;
}

inline uint64_t where_list_bytes(const WhereShape& s, uint64_t m) { return m * (uint64_t)s.ld * 4; }

inline uint64_t where_mask_bytes(const WhereShape& s)
{
    const uint64_t row = s.first_stage == WHERE_STAGE_I8 ? (uint64_t)s.ldb : s.first_stage == WHERE_STAGE_BF16 ? 2 * (uint64_t)s.ldb : 4 * (uint64_t)s.ld;
    return s.len * row;
}

// true: the masked ladder; false: the position list
inline bool where_route_mask(int mode, const WhereShape& s, uint64_t m, uint64_t k)
{
    if (mode == WHERE_ROUTE_LIST || !where_mask_eligible(s, m, k)) return false;
    if (mode == WHERE_ROUTE_MASK) return true;
    return where_mask_bytes(s) < where_list_bytes(s, m);
}

}  // namespace vl
