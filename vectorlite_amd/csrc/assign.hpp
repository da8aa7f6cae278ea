// assign.hpp -- launch interface of the nearest-label assignment's kernels (assign.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assign_plan.hpp"
#include "kernels.hpp"

namespace vl {

constexpr int ASSIGN_CTR_CAND = 0;  // candidate pairs of the range (counts past the buffer: the host splits the range)
constexpr int ASSIGN_CTR_NAN = 1;   // a reference score is NaN
constexpr int ASSIGN_CTR_WORDS = 4;

struct AssignSeed {  // the first pass' answer for one row
    float key;
    uint32_t label;
};
struct AssignCand {  // a pair the second pass kept; k_assign_pairs fills in the score
    uint32_t row, label;
    double score;
};

// The per-range arrays, indexed by (storage position - 32 b0); each holds 32 (b1 - b0) entries.
struct AssignRows {
    AssignSeed* seeds;          // pass 0 -> k_assign_seed
    double* S;                  // the seed's reference score
    float* thr;                 // the row's threshold of the second pass
    uint32_t* seed_label;
    unsigned long long* best;   // assign_score_enc of the best score seen (fetch-max)
    uint32_t* winner;           // (label << 1 | the score is -0.0) of the lowest label that reaches best (fetch-min)
    unsigned long long* out_labels;
    double* out_scores;
};

// cosine / dot / Euclidean at a stride the row-stationary slab has (128 .. 768)
bool assign_rows_supported(uint32_t dim, int metric);

// a[c], b_seed[c], b_keep[c] of assign_label for the labels' norms; entries n_labels .. n_pad are padding labels that no row
// keeps (a = 0, b = -inf).  n_pad = whole chunks.
hipError_t launch_assign_labels(hipStream_t s, int metric, const double* label_norms, uint32_t n_labels, uint32_t n_pad, uint32_t ldb,
                                double R, float* a, float* b_seed, float* b_keep);

// k_assign_rows over the blocks [r.b0, r.b1).  q_bf16: the labels' bf16 image, zero rows up to n_pad; a / b: the scalars of
// the mode (b_seed for mode 0, b_keep for mode 1).  Mode 0 writes rows.seeds; mode 1 reads rows.thr and rows.seed_label and
// appends to cand (cap entries), counting in ctr[ASSIGN_CTR_CAND].
hipError_t launch_assign_rows(hipStream_t s, int metric, int mode, const void* slab_frag, const float* row_norm, const void* q_bf16,
                              const float* a, const float* b, uint32_t n_labels, uint64_t n_rows, uint32_t dim, AssignRange r,
                              const AssignRows& rows, AssignCand* cand, uint32_t cap, uint32_t* ctr);

// S, thr, seed_label, best and winner of the range's rows from the seeds (the reference's f64 arithmetic in index order)
hipError_t launch_assign_seed(hipStream_t s, int metric, const double* master, const double* labels64, const float* row_sqnorm,
                              uint32_t n_labels, uint64_t n_rows, uint32_t dim, AssignRange r, const AssignRows& rows, uint32_t* ctr);

// The tail of a range: the exact score of every kept pair raises best[row]; the lowest label among the pairs and the seed
// that reach it wins; out_labels / out_scores carry the winner and its own score bits.  Nothing when the counter ran past cap.
hipError_t launch_assign_finish(hipStream_t s, int metric, const double* master, const double* labels64, uint32_t n_labels,
                                uint64_t n_rows, uint32_t dim, AssignRange r, const AssignRows& rows, AssignCand* cand, uint32_t cap,
                                uint32_t* ctr);

// The exact route, one label: (best[p], label[p]) <- (scores[p], l) where scores[p] is strictly greater in the contract's
// order (always for l == 0); a NaN score sets ctr[ASSIGN_CTR_NAN].
hipError_t launch_assign_fold(hipStream_t s, const double* scores, uint64_t n_rows, uint32_t l, double* best, uint32_t* label,
                              uint32_t* ctr);

}  // namespace vl
