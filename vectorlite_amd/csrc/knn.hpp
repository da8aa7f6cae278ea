// knn.hpp -- launch interface of the k-nearest-neighbour graph's kernels (knn.hip); the ranking of the
// records runs on kernels.hip's bitonic network (launch_knn_rank).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knn_plan.hpp"

namespace vl {

constexpr int KNN_CTR_CAND = 0;  // kept pairs of the range (counts past the buffer: the host splits the range)
constexpr int KNN_CTR_NAN = 1;   // a reference score is NaN
constexpr int KNN_CTR_WORDS = 4;

struct KnnCand {  // a pair the keep pass kept
    uint32_t row, col;
};

// A record's sort payload.  The record's key is its row; within a row the payload orders by (score desc with -0.0 == +0.0,
// partner asc).  neg_zero keeps the sign that dkey folds away.
struct KnnPay {
    unsigned long long dkey;  // desc_key(score)
    uint32_t partner;
    uint32_t neg_zero;
    __host__ __device__ bool operator>(const KnnPay& o) const { return dkey > o.dkey || (dkey == o.dkey && partner > o.partner); }
    __host__ __device__ bool operator==(const KnnPay& o) const { return dkey == o.dkey && partner == o.partner; }
};

// The per-range arrays; rows are indexed by (storage position - 32 b0), a range holds rr = 32 (b1 - b0) of them.
struct KnnRows {
    uint32_t* seeds;               // [rr][k] the seed pass' partners
    float* thr;                    // [rr] the keep pass' threshold (+inf past the last row)
    unsigned long long* rec_keys;  // [sort_capacity_for(rr k + cap)] records: the seeds' first, the kept pairs' behind
    KnnPay* rec_pay;
    uint32_t* out_pos;             // [rr][kk]
    double* out_scores;            // [rr][kk]
};

// cosine / dot / Euclidean at a stride the fragment-major slab has (128 .. 768)
bool knn_rows_supported(uint32_t dim, int metric);

// k_knn_rows over the blocks [r.b0, r.b1) against every stored row.  Mode 0 writes rows.seeds (k distinct partners per row,
// the self pair never among them; needs n_rows - 1 >= k).  Mode 1 reads rows.thr and appends every (row, column != row)
// whose key test reaches the row's threshold to cand (cap entries), counting in ctr[KNN_CTR_CAND].
hipError_t launch_knn_rows(hipStream_t s, int metric, int mode, const void* slab_frag, const float* row_norm, uint64_t n_rows,
                           uint32_t dim, AssignRange r, uint32_t k, const KnnRows& rows, KnnCand* cand, uint32_t cap, uint32_t* ctr);

// The seeds' reference scores (row p the query, Acc64 in index order) as the range's first rr k records, and thr[p] = the
// join's threshold for min_score = S_p, the k-th largest seed score.  R = the largest row norm.
hipError_t launch_knn_seed(hipStream_t s, int metric, const double* master, uint64_t n_rows, uint32_t dim, AssignRange r, uint32_t k,
                           double R, const KnnRows& rows, uint32_t* ctr);

// The kept pairs' reference scores as the records behind the seeds'.  Nothing when the counter ran past cap.
hipError_t launch_knn_pairs(hipStream_t s, int metric, const double* master, uint64_t n_rows, uint32_t dim, AssignRange r, uint32_t k,
                            const KnnRows& rows, const KnnCand* cand, uint32_t cap, uint32_t* ctr);

// Sorts the first `total` records by (row, score desc, partner asc); the buffers hold sort_capacity_for(total) entries.
// (kernels.hip)
hipError_t launch_knn_rank(hipStream_t s, unsigned long long* rec_keys, KnnPay* rec_pay, uint64_t total);

// Per row of the range the first kk distinct partners of its sorted records, with their own score bits; an entry the
// records cannot fill is 0xFFFFFFFF.
hipError_t launch_knn_emit(hipStream_t s, uint64_t n_rows, AssignRange r, uint32_t kk, uint64_t total, const KnnRows& rows);

}  // namespace vl
