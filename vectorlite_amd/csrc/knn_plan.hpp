// knn_plan.hpp -- the k-nearest-neighbour graph of the stored rows (knn.hip): the limits of the pass,
// its column chunk, and how the candidate buffer sizes the row ranges.  The range stack itself is the assignment's
// (assign_ranges / assign_split, assign_plan.hpp); the key tests are the join's (join_plan.hpp).
// Plain C++ (host and device).
#pragma once

#include <stdint.h>

#include "assign_plan.hpp"

namespace vl {

constexpr uint32_t KNN_MAX_K = 32;           // VL_KNN_MAX_K: entries of a row's list in LDS
constexpr uint32_t KNN_BLOCK_ROWS = 32;      // rows of one wave's block: the unit of a row range
constexpr uint32_t KNN_CAND_CAP = 1u << 22;  // kept pairs of one range (a guess, not a measurement)
static_assert(KNN_BLOCK_ROWS == ASSIGN_BLOCK_ROWS, "the ranges are the assignment's");

// Rows of the slab per column chunk at a bf16 row stride: one chunk (two up to stride 256) lies in LDS next to the eight
// waves' lists (64 KB) and rings: 64 x 1024 B at stride 512, 48 x 1536 B at stride 768.
constexpr uint32_t knn_chunk(uint32_t ldb) { return ldb <= 512 ? 64u : 48u; }

// Every seed is kept again by the second pass (its score reaches the row's S), so a block keeps at least 32 k pairs: a
// buffer below that could not hold one block's seeds, and a single block would overflow whatever the data.
inline uint32_t knn_cap(uint32_t cap, uint32_t k)
{
    const uint32_t floor = KNN_BLOCK_ROWS * k;
    return cap < floor ? floor : cap;
}

// blocks of the first ranges: four kept pairs per seed (a guess; nothing was measured).  An overflowing range is halved.
inline uint32_t knn_range_blocks(uint32_t cap, uint32_t k)
{
    const uint32_t b = cap / (4u * k) / KNN_BLOCK_ROWS;
    return b < 1u ? 1u : b;
}

}  // namespace vl
