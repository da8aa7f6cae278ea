// mmr_batch_plan.hpp -- does a batch of diversified (MMR) queries take the MFMA pass with the rank / similarity / selection
// stage or the loop over the single diversified search (section 16)?  Pure host arithmetic (no device
// code): tests/native/mmr_batch_plan_test.cpp checks the properties below on the CPU; flat_index.cpp (search_mmr_batch)
// fills the shape in and asks.
//
//   M1  mode 0 (off) never takes the pass; an input that is not eligible never takes it in any mode
//   M2  mode 1 (on) takes it whenever the input is eligible
//   M3  mode 2 (auto) takes it iff the pass's estimated time is below the loop's
//   M4  both estimates are nondecreasing in the number of queries; the loop estimate is nondecreasing in m = |S| under an
//       include token and does not depend on it otherwise; the pass estimate never depends on it
//   M5  the decision is a function of its arguments
//
// BOTH ESTIMATES ARE DERIVED from constants measured on other routes, not fitted to this one (nothing of this route had
// been measured when the rule was written):
//   the pass:  masked_batch_plan.hpp's estimate per launch sequence (its constants were measured on the masked pass; the
//              unmasked pass of an unfiltered call is not slower).  The MMR stage behind the rescoring and the queries the
//              pass hands back to the single call are NOT charged: the hand-back rate depends on the data;
//   the loop:  nq x the bytes of the cheapest stage the single call could START with on this index, at the rate README.md
//              records for that stage, and nothing else -- no later stage of the ladder, no tail (27-52 us per call), no
//              launch cost.  Unfiltered or under an exclusion token that is the single-query ladder's first stage by its
//              own size thresholds on the f32 slab: the int8 copy (dim bytes per row, k_scan_i8 6.75 TB/s), the bf16 copy
//              (ldb x 2 bytes, k_scan_bf16 7.0 TB/s) or the f32 slab (ld x 4 bytes, k_scan 6.99 TB/s).  Under an include
//              token it is the subset scan over the token's m rows, m x ld x 4 bytes at k_scan_subset's best rate
//              (7.0 TB/s).  Every choice favours the loop, the route that was there before.
// So at 10 M x 384 two unfiltered queries loop (2 x 0.57 ms against 3.8 ms for a sequence) and seven take the pass; README
// has the single call at 0.647 ms and a 256-query pass at 1.9 ms, so the measured crossover lies lower (two to three
// queries).  Under a 1 % include token the loop is charged 22 us per query and wins up to 175 queries (measured single
// call: 92 us, crossover near fifteen to twenty).
// What tools/mmr_batch_probe.py measured since (one run, profiles/mmr_batch_10000000x384.jsonl, (4, 20)): the loop costs
// 0.65 ms per query unfiltered and 99 us under a 1 % include token, the pass 1.4 / 2.0 / 17.5 ms for 16 / 256 / 2048
// queries; at 16 queries under the include token the two routes are level (1.55 against 1.58 ms) and "auto" loops.  The
// constants have NOT been refitted to that run.
#pragma once

#include <stdint.h>

#include <algorithm>

#include "masked_batch_plan.hpp"

namespace vl {

enum : int { MMR_BATCH_OFF = 0, MMR_BATCH_ON = 1, MMR_BATCH_AUTO = 2 };

constexpr double MMR_LOOP_I8_BYTES_PER_US = 6.75e6;
constexpr double MMR_LOOP_BF16_BYTES_PER_US = 7.0e6;
constexpr double MMR_LOOP_F32_BYTES_PER_US = 6.99e6;
constexpr double MMR_LOOP_SUBSET_BYTES_PER_US = 7.0e6;

struct MmrBatchShape {
    MaskedBatchShape index;   // index_ok: no forced path, no out-of-domain row, mfma_scan_supported(dim, metric)
    bool rows_kernel;         // mfma_rows_kernel(dim): what the masked pass needs
    bool filtered;            // a token of either kind: the masked pass under a keep bitmap
    bool include;             // an include token: the single call scans the token's m rows only
    uint64_t m;               // |S|: the rows the filter keeps (len without a filter)
    uint64_t i8_min_bytes;    // the ladder's thresholds on the f32 slab's bytes: the int8 stage from here on,
    uint64_t bf16_min_bytes;  // the bf16 stage from here on, the f32 scan below
};

// masked_query_eligible's conditions with n = min(fetch_k, m) inside the list's margin, and the batch's own: two or more
// queries, and the masked kernel where a bitmap is needed
inline bool mmr_batch_eligible(const MmrBatchShape& s, const MaskedBatchLimits& lim, uint64_t nq, uint64_t fetch_k)
{
    if (fetch_k == 0 || !masked_query_eligible(s.index, lim, s.m, fetch_k)) return false;
    if (s.filtered && !s.rows_kernel) return false;
    return s.m <= s.index.len && nq >= lim.min_batch && nq > 0;
}

inline double mmr_loop_estimate_us(const MmrBatchShape& s, uint64_t nq)
{
    double per_query;
    if (s.include) {
        per_query = (double)s.m * (double)s.index.ld * 4.0 / MMR_LOOP_SUBSET_BYTES_PER_US;
    } else {
        const uint64_t slab = s.index.len * (uint64_t)s.index.ld * 4;
        if (slab >= s.i8_min_bytes) per_query = (double)s.index.len * (double)s.index.dim / MMR_LOOP_I8_BYTES_PER_US;
        else if (slab >= s.bf16_min_bytes) per_query = (double)s.index.len * (double)s.index.ldb * 2.0 / MMR_LOOP_BF16_BYTES_PER_US;
        else per_query = (double)slab / MMR_LOOP_F32_BYTES_PER_US;
    }
    return (double)nq * per_query;
}

inline double mmr_pass_estimate_us(const MmrBatchShape& s, const MaskedBatchLimits& lim, uint64_t nq)
{
    return masked_mfma_estimate_us(s.index, lim, nq);
}

inline bool mmr_batch_route(int mode, const MmrBatchShape& s, const MaskedBatchLimits& lim, uint64_t nq, uint64_t fetch_k)
{
    if (mode == MMR_BATCH_OFF || !mmr_batch_eligible(s, lim, nq, fetch_k)) return false;
    if (mode == MMR_BATCH_ON) return true;
    return mmr_pass_estimate_us(s, lim, nq) < mmr_loop_estimate_us(s, nq);
}

}  // namespace vl
