// grouped_batch_plan.hpp -- does a batch of grouped queries take the MFMA pass with the rank-and-collapse stage (DESIGN.md
// section 26) or the loop over the single grouped search (section 18)?  Pure host arithmetic (no device code):
// tests/native/grouped_batch_plan_test.cpp checks the properties below on the CPU; flat_index.cpp (search_grouped_batch)
// fills the shape in and asks.
//
//   G1  mode 0 (off) never takes the pass; an input that is not eligible never takes it in any mode
//   G2  mode 1 (on) takes it whenever the input is eligible
//   G3  mode 2 (auto) takes it iff the pass's estimated time is below the loop's
//   G4  both estimates are nondecreasing in the number of queries; the loop estimate is nondecreasing in m = |S|, the
//       pass estimate does not depend on it
//   G5  the decision is a function of its arguments
//
// BOTH ESTIMATES ARE DERIVED from constants measured on other routes, not fitted to this one:
//   the pass:  masked_batch_plan.hpp's estimate per launch sequence (its constants were measured on the masked pass the
//              filtered route runs here; the unmasked pass of a table that covers every row is not slower).  Queries the
//              pass hands back to the single call are NOT charged: the hand-back rate depends on the data;
//   the loop:  per query two streaming passes over the m rows of S (k_scan_group_best, then k_scan_range / k_scan_subset),
//              nq x 2 x m x ld x 4 bytes, at the best rate README.md records for those scans (k_scan_range: 7.05 TB/s
//              over the whole index; k_scan_subset: 5.2-7.0 TB/s).  The higher rate is used, and the atomics of
//              k_scan_group_best are not charged -- both favour the route that was there before.
// What tools/grouped_batch_probe.py measured at 10 M x 384 (cosine, k = 10, one MI355X, wall time per call,
// profiles/grouped_batch_10000000x384.jsonl): the loop costs 4.8 ms per query when every row has a group (estimate: 4.4)
// and 3.0 ms at 60 % grouped (2.6); the pass 1.3 / 1.8-2.1 / 12.1-13.2 ms for 16 / 256 / 2048 queries (estimate: 3.8 /
// 3.8 / 20.4).  Both estimates err towards the loop, and "auto" took the faster route in all nine records.  Where the two
// routes cross (an S of a few ten thousand rows at 256 queries) is still unmeasured.
#pragma once

#include <stdint.h>

#include <algorithm>

#include "masked_batch_plan.hpp"

namespace vl {

enum : int { GROUPED_BATCH_OFF = 0, GROUPED_BATCH_ON = 1, GROUPED_BATCH_AUTO = 2 };

constexpr double GROUPED_LOOP_BYTES_PER_US = 7.05e6;

struct GroupedBatchShape {
    MaskedBatchShape index;  // index_ok: no forced path, no out-of-domain row, mfma_scan_supported(dim, metric)
    bool rows_kernel;        // mfma_rows_kernel(dim): what the masked pass needs
    bool needs_bitmap;       // a filter, or rows without a group: the masked pass under the keep bitmap of S
    uint64_t m;              // |S|: the rows with a group that the filter keeps
};

// the conditions masked_query_eligible asks of a query, with the batch's own: k itself within the list's margin (a
// grouped answer of k groups needs at least k candidates whatever m is), and the masked kernel where a bitmap is needed
inline bool grouped_batch_eligible(const GroupedBatchShape& s, const MaskedBatchLimits& lim, uint64_t nq, uint64_t k)
{
    if (!masked_query_eligible(s.index, lim, s.m, k) || k > lim.k_max || k == 0) return false;
    if (s.needs_bitmap && !s.rows_kernel) return false;
    return s.m <= s.index.len && nq >= lim.min_batch && nq > 0;
}

inline double grouped_loop_estimate_us(const GroupedBatchShape& s, uint64_t nq)
{
    return (double)nq * 2.0 * (double)s.m * (double)s.index.ld * 4.0 / GROUPED_LOOP_BYTES_PER_US;
}

inline double grouped_pass_estimate_us(const GroupedBatchShape& s, const MaskedBatchLimits& lim, uint64_t nq)
{
    return masked_mfma_estimate_us(s.index, lim, nq);
}

inline bool grouped_batch_route(int mode, const GroupedBatchShape& s, const MaskedBatchLimits& lim, uint64_t nq, uint64_t k)
{
    if (mode == GROUPED_BATCH_OFF || !grouped_batch_eligible(s, lim, nq, k)) return false;
    if (mode == GROUPED_BATCH_ON) return true;
    return grouped_pass_estimate_us(s, lim, nq) < grouped_loop_estimate_us(s, nq);
}

}  // namespace vl
