// join.hpp -- launch interface of the similarity self-join: the candidate pass (join.hip) and the
// rescore / cut / rank / emit tail (kernels.hip, next to rescore_rows_par's arithmetic and the bitonic network it reuses).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "join_plan.hpp"

namespace vl {

// a candidate pair of storage positions a < b and its bf16 key
struct JoinCand {
    uint32_t a, b;
    float key;
};

// a survivor's sort payload: the pair (a << 32 | b decides ties between equal scores) and the score's own bits
struct JoinPay {
    unsigned long long ab, bits;
    __host__ __device__ bool operator>(const JoinPay& o) const { return ab > o.ab; }
    __host__ __device__ bool operator==(const JoinPay& o) const { return ab == o.ab; }
};

struct JoinLaunchInfo {
    int ksteps = 0;      // k_join_rows<KSTEPS>
    int grid = 0;        // workgroups
    uint64_t units = 0;  // (panel, block) units of the launch
};

// rows of this length have a k_join_rows shape for the metric (cosine, Euclidean, dot; the fragment-major slab's strides
// 128 .. 768)
bool join_rows_supported(uint32_t dim, int metric = 0 /* COSINE */);

// The pass over the panels [y0, y1) of join_plan(n_rows, join_qpb(mfma_ldb(dim))): *cnt is cleared (by a kernel) and then
// counts every pair a < b < n_rows with a column in those panels whose key reaches thr; the first `cap` of them (in no
// particular order) are written to cand.  *cnt > cap: the range has to be split.  Cosine compares the bf16 key itself
// (join_key_threshold); Euclidean and dot compare join_pair_key of the key and the two rows' norm16 entries (row_norm) with
// join_pair_threshold's scalar.  The candidate carries the cosine key for every metric.
hipError_t launch_join_rows(hipStream_t s, int metric, const void* slab_frag, const float* row_norm, uint64_t n_rows, uint32_t dim,
                            uint32_t y0, uint32_t y1, float thr, JoinCand* cand, uint32_t* cnt, uint32_t cap,
                            JoinLaunchInfo* info = nullptr);

// ctr: JOIN_CTR_WORDS 64-bit words, zeroed (launch_join_clear) in front of a call's first range.
constexpr int JOIN_CTR_TOTAL = 0, JOIN_CTR_NAN = 1, JOIN_CTR_WORDS = 2;
hipError_t launch_join_clear(hipStream_t s, unsigned long long* ctr);
// Rescore + cut of one range's candidates (cosine, Euclidean or dot; nothing is done when *cnt > cap): tiles of 16 pairs in
// the reference's f64 order, row a as the query; pairs with score >= min_score are appended as (desc_key(score), {a << 32 | b, score bits})
// while they fit sv_cap; ctr[TOTAL] counts them all, ctr[NAN] is raised by a NaN score.
hipError_t launch_join_rescore_cut(hipStream_t s, int metric, const JoinCand* cand, const uint32_t* cnt, uint32_t cap, const double* master,
                                   uint32_t dim, uint64_t n_rows, double min_score, unsigned long long* sv_keys, JoinPay* sv_pay,
                                   uint64_t sv_cap, unsigned long long* ctr);
// Sorts the first `total` survivors (total <= sv_cap; the buffers hold sort_capacity_for(total) entries) by (score desc with
// -0.0 == +0.0, a asc, b asc) on k_bitonic_local / k_bitonic_global's network.
hipError_t launch_join_rank(hipStream_t s, unsigned long long* sv_keys, JoinPay* sv_pay, uint64_t total);

}  // namespace vl
