// masked_batch_plan.hpp -- does a batch of exclusion-filtered queries take the mask-aware MFMA pass
// or the jobs kernel (section 14)?  Pure host arithmetic (no HIP): tests/native/masked_batch_plan_test.cpp checks the
// properties below on the CPU; flat_index.cpp (search_batch_filters) collects the eligible queries and asks.
//
//   R1  mode 0 (off) never takes the masked route; an input that is not eligible never takes it in any mode
//   R2  mode 1 (on) takes it whenever the input is eligible
//   R3  mode 2 (auto) takes it iff the masked route's estimated time is below the jobs route's
//   R4  both estimates are nondecreasing in the number of queries and in the index length; the jobs estimate is
//       nondecreasing in every m_q, the masked estimate does not depend on them
//   R5  the decision is a function of its arguments
#pragma once

#include <stdint.h>

#include <algorithm>

namespace vl {

enum : int { MASKED_BATCH_OFF = 0, MASKED_BATCH_ON = 1, MASKED_BATCH_AUTO = 2 };

// The rates of the cost rule, from tools/exclude_batch_probe.py's quick run at 10 M x 384 (cosine, k = 10, 256 queries, one
// MI355X, profiles/exclude_batch_10000000x384.jsonl; HIP-event kernel times unless said otherwise):
//   jobs kernel:  256 lists of 50 000 rows in 2.33 ms = 8.4 TB/s of f32 rows (6.8 TB/s on lists of 5 M rows: the higher
//                 rate is used -- it favours the route that was there before);
//   masked pass:  7.68 GB of bf16 rows in 2.0 ms when half the rows are kept = 3.8 TB/s (the unfiltered batch beside it:
//                 1.9-2.0 ms), 2.4 ms when 5 % are kept, 3.5 ms when 0.5 % are: thresholds sampled from few kept rows are
//                 loose and the candidate code runs more often.  The rule charges the worst measured factor, 1.8, always;
//   tail:         wall time minus kernel time of a call, 0.15-0.27 ms;
//   flop rate:    NOT measured on the masked pass (the quick run holds no 2048-query record): derived from the unmasked
//                 batch's 22.5 ms for 4096 queries = 1.4 PFLOP/s.
// Measured crossover at 256 queries: the jobs route wins at 0.5 % kept (2.46 against 3.69 ms per call), the masked pass at
// 5 % (2.64 against 28.2 ms); the rule puts it at 0.8 %.  256 distinct bitmaps cost the pass 0.7 ms more than one shared
// bitmap (2.93 against 2.15 ms per call), inside the factor above.
constexpr double MASKED_JOBS_BYTES_PER_US = 8.4e6;
constexpr double MASKED_MFMA_BYTES_PER_US = 3.8e6;
constexpr double MASKED_MFMA_FLOP_PER_US = 1.4e9;
constexpr double MASKED_SPARSE_FACTOR = 1.8;
constexpr double MASKED_SEQUENCE_TAIL_US = 200.0;

struct MaskedBatchLimits {
    uint64_t min_rows;     // MFMA_MIN_ROWS: shorter indexes leave the sampling pass without a threshold
    uint64_t min_batch;    // MFMA_MIN_BATCH
    uint64_t k_max;        // KFAST_MAX: the 64-entry list must keep a margin
    uint32_t seq_queries;  // mfma_sequence_queries(dim): queries one launch sequence answers
};

struct MaskedBatchShape {
    bool index_ok;   // no forced path, no out-of-domain row, the row-stationary kernel has a shape for (dim, metric)
    uint64_t len;    // rows of the index
    uint32_t dim;
    uint32_t ld;     // f32 row stride (the jobs kernel's rows)
    uint32_t ldb;    // bf16 row stride (the MFMA filter's rows)
};

// one query's side of the eligibility: its filter keeps m rows, the call asks for k
inline bool masked_query_eligible(const MaskedBatchShape& s, const MaskedBatchLimits& lim, uint64_t m, uint64_t k)
{
    return s.index_ok && s.len >= lim.min_rows && m > 0 && std::min<uint64_t>(k, m) <= lim.k_max;
}

// microseconds of the jobs route for the eligible queries: sum_m = the sum of their m_q
inline double masked_jobs_estimate_us(const MaskedBatchShape& s, uint64_t sum_m)
{
    return (double)sum_m * (double)s.ld * 4.0 / MASKED_JOBS_BYTES_PER_US;
}

// microseconds of the masked MFMA route for nq eligible queries: whole sequences, each bound by its rows or by its flops
inline double masked_mfma_estimate_us(const MaskedBatchShape& s, const MaskedBatchLimits& lim, uint64_t nq)
{
    const uint64_t seq = std::max<uint32_t>(lim.seq_queries, 1);
    double us = 0.0;
    for (uint64_t q0 = 0; q0 < nq; q0 += seq) {
        const uint64_t g = std::min<uint64_t>(seq, nq - q0);
        const double rows_us = (double)s.len * (double)s.ldb * 2.0 / MASKED_MFMA_BYTES_PER_US;
        const double flop_us = 2.0 * (double)g * (double)s.len * (double)s.dim / MASKED_MFMA_FLOP_PER_US;
        us += std::max(rows_us, flop_us) * MASKED_SPARSE_FACTOR + MASKED_SEQUENCE_TAIL_US;
    }
    return us;
}

// n_eligible queries passed masked_query_eligible, their filters keep sum_m rows in all
inline bool masked_batch_route(int mode, const MaskedBatchShape& s, const MaskedBatchLimits& lim, uint64_t n_eligible, uint64_t sum_m)
{
    if (mode == MASKED_BATCH_OFF || !s.index_ok || s.len < lim.min_rows) return false;
    if (n_eligible == 0 || n_eligible < lim.min_batch) return false;
    if (mode == MASKED_BATCH_ON) return true;
    return masked_mfma_estimate_us(s, lim, n_eligible) < masked_jobs_estimate_us(s, sum_m);
}

}  // namespace vl
