// examples.hpp -- launch interface of the search by positive and negative examples (examples.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "examples_plan.hpp"
#include "kernels.hpp"

namespace vl {

// counters of one call (device words, zeroed by the caller)
constexpr int EXAMPLES_CTR_SEEDS = 0;      // min(64, rows): the rows scored in the first round
constexpr int EXAMPLES_CTR_SURVIVORS = 1;  // rows with U >= L (counts past the cap)
constexpr int EXAMPLES_CTR_NAN = 2;        // a reference score of (example, stored row) is NaN
constexpr int EXAMPLES_CTR_WORDS = 4;

struct ExamplesRowsInfo {
    int ksteps = 0, blocks = 0, grid_x = 0;
};

// cosine / dot / Euclidean at a stride the row-stationary slab has (128 .. 768)
bool examples_rows_supported(uint32_t dim, int metric);

// map[c], c < 16 (blocks(a) + blocks(b)): the (a, c) pair of image column c from the staged norms q_norms[0 .. a + b);
// *q_max = the largest norm among the positives
hipError_t launch_examples_map(hipStream_t s, int metric, const double* q_norms, uint32_t a, uint32_t b, ExamplesMap* map,
                               double* q_max);

// The candidate pass, one launch over every row: K[p] = (max over the positives, max over the negatives) of the mapped keys
// of row p; the second is -inf when b == 0.  q_bf16: the image, [16 (blocks(a) + blocks(b)), ldb] bf16 rows in the block
// layout of examples_plan.hpp, zero rows for padding; slab_frag, row_norm, row_sqnorm: the fragment-major slab and its
// per-row arrays.  Rows at or past n_rows are not written.
hipError_t launch_examples_rows(hipStream_t s, int metric, const void* slab_frag, const float* row_norm, const float* row_sqnorm,
                                const void* q_bf16, const ExamplesMap* map, uint32_t a, uint32_t b, uint64_t n_rows, uint32_t dim,
                                float2* K, ExamplesRowsInfo* info);

// The 64 rows of largest estimated f (an f32 reading of K, no rigour): top[0 .. c), ctr[SEEDS] = c = min(64, n_rows).
// lists: EXAMPLES_TOP_LISTS * KP entries of scratch.
hipError_t launch_examples_seed(hipStream_t s, int metric, const float2* K, uint64_t n_rows, bool has_neg, Cand32* lists,
                                uint32_t* top, uint32_t* ctr);

// f[i] of the rows list[0 .. *n_list), in the reference's f64 arithmetic: every (row, example) score, the ordered maximum
// per side (-0.0 below +0.0), f = P when b == 0 or P > N, else -(N N).  q64: [a + b, dim], positives first.  ctr[NAN] is
// set by a NaN score.  Nothing is scored when *n_list exceeds cap.
hipError_t launch_examples_exact(hipStream_t s, int metric, const double* master, const double* q64, uint32_t a, uint32_t b,
                                 uint32_t dim, const uint32_t* list, const uint32_t* n_list, uint32_t cap, uint64_t n_rows,
                                 double* f, uint32_t* ctr);

// Every row whose U (examples_upper of K[p].x; ldb, R, *q_max, IN_EXTRA_MFMA) is not below L: list[i] = p for the first
// `cap` of them, in no particular order; ctr[SURVIVORS] counts them all.
hipError_t launch_examples_survivors(hipStream_t s, int metric, const float2* K, uint64_t n_rows, bool has_neg, uint32_t ldb,
                                     double R, const double* q_max, double L, uint32_t cap, uint32_t* list, uint32_t* ctr);

// The first min(k, *n_list) of list[0 .. *n_list) by (f desc, position asc) -> out_pos, out_f.  Nothing when *n_list exceeds
// cap <= EXAMPLES_CAND_CAP.
hipError_t launch_examples_rank(hipStream_t s, const uint32_t* list, const double* f, const uint32_t* n_list, uint32_t cap,
                                uint32_t k, uint32_t* out_pos, double* out_f);

// The exact route.  fold: acc[p] = scores[p] for the side's first example, the ordered maximum of the two after it;
// ctr[NAN] is set by a NaN score.  fuse: f[p] from P[p] and N[p] (N == nullptr: no negatives).
hipError_t launch_examples_fold(hipStream_t s, const double* scores, uint64_t n_rows, bool first, double* acc, uint32_t* ctr);
hipError_t launch_examples_fuse(hipStream_t s, const double* P, const double* N, uint64_t n_rows, double* f);

}  // namespace vl
