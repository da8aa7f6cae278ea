// deep_batch.hpp -- launch interface of the deep-k batch (deep_batch.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deep_batch_plan.hpp"
#include "kernels.hpp"

namespace vl {

// cosine / dot / Euclidean at a stride the row-stationary slab has (128 .. 768)
bool deep_sample_supported(uint32_t dim, int metric);

// The sampling pass: group maxima over 8 rows of `sample_blocks` 32-row blocks spread evenly over the index
// (deep_sample_block), 4 per block and query: gm[(4 i + g) * nq_pad + q], i = the sample block, g = its 8-row group.
// q_bf16: [nq_pad, ldb] bf16 queries in whole chunks of k_mfma_rows (zero rows for padding); slab_frag, row_norm,
// row_sqnorm: the fragment-major slab and its per-row arrays.  Rows at or past n_rows count as -inf.
hipError_t launch_deep_sample(hipStream_t s, int metric, const void* slab_frag, const float* row_norm, const float* row_sqnorm,
                              const void* q_bf16, uint32_t nq_pad, uint32_t sample_blocks, uint64_t n_rows, uint32_t dim, float* gm);

// thr[q] = max(mask[q], the K-th largest of gm[g * nq_pad + q], g < n_groups); K <= n_groups <= DEEP_SELECT_MAX.
// mask[q] = -inf for a query the route answers, +inf for one it must not collect candidates for.
hipError_t launch_deep_select_sample(hipStream_t s, const float* gm, uint32_t nq_pad, uint32_t n_groups, uint32_t K, uint32_t nq,
                                     const float* mask, float* thr);

// Per query q with cnt[q] <= cap <= DEEP_SELECT_MAX entries cand[q * cap ..]: T = the K-th largest key (K == 0: T =
// thr[q] as it stands; fewer than K entries: T = thr[q], nothing else happens).  thr[q] = T (write_thr), and every entry
// with key >= T -- all ties with T -- moves to the front of dst[q * dst_cap ..] in its order, dst_cnt[q] = their number
// (dst_cap + 1 when they do not fit dst_cap; dst == cand compacts in place).  A query whose counter exceeds cap (the
// buffer or a ring segment overflowed) is left alone: thr[q] = +inf (write_thr), dst_cnt[q] = dst_cap + 1 (dst != cand).
hipError_t launch_deep_select(hipStream_t s, const Cand32* cand, uint32_t* cnt, uint32_t cap, uint32_t nq, uint32_t K, float* thr,
                              bool write_thr, Cand32* dst, uint32_t* dst_cnt, uint32_t dst_cap);

// out[q] = thr[q] for the queries whose index within their chunk of qpb is congruent to `a` modulo `A`, +inf for the rest
hipError_t launch_deep_stripe(hipStream_t s, const float* thr, uint32_t nq, uint32_t qpb, uint32_t A, uint32_t a, float* out);

// L[q] = the smallest of scores[q * seg + i], i < total[q * ctr_words] (the seeds' exact scores); NaN when a score is NaN,
// the query has no seeds or more than seg
hipError_t launch_deep_seed_min(hipStream_t s, const double* scores, uint32_t seg, const uint32_t* total, uint32_t ctr_words,
                                uint32_t nq, double* L);

// words[0 .. n) = 0 (a launch sequence's counters)
hipError_t launch_deep_clear(hipStream_t s, uint32_t* words, uint32_t n);

}  // namespace vl
