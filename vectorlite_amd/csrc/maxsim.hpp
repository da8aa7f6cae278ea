// maxsim.hpp -- launch interface of the late-interaction (MaxSim) search's kernels (maxsim.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "maxsim_plan.hpp"

namespace vl {

// counters of one call (device words, cleared by launch_maxsim_clear)
constexpr int MAXSIM_CTR_GROUPS = 0;     // groups that hold a row
constexpr int MAXSIM_CTR_TOP = 1;        // min(64, those): the groups scored in the first round
constexpr int MAXSIM_CTR_SURVIVORS = 2;  // groups with U >= L (counts past the cap)
constexpr int MAXSIM_CTR_MEMBERS = 3;    // member rows of the round's groups (counts past the cap)
constexpr int MAXSIM_CTR_NAN = 4;        // a reference score over a grouped row is NaN
constexpr int MAXSIM_CTR_WORDS = 8;
constexpr uint32_t MAXSIM_NO_CAND = 0xFFFFFFFFu;
constexpr int MAXSIM_TOP_LISTS = 64;
constexpr unsigned long long MAXSIM_EMPTY_BITS = ~0ull;  // the exact route's accumulator of a group without a row

struct MaxsimMember {
    uint32_t cand;  // index into the round's group list
    uint32_t pos;   // storage position
};

struct MaxsimRowsInfo {
    int ksteps = 0, chunks = 0, grid_x = 0;
};

// cosine / dot / Euclidean at a stride the row-stationary slab has (128 .. 768)
bool maxsim_rows_supported(uint32_t dim, int metric);

// p[0..n) = v; ctr[0..MAXSIM_CTR_WORDS) = 0 (kernels: a launch sequence holds no memset node)
hipError_t launch_maxsim_fill(hipStream_t s, uint32_t* p, uint64_t n, uint32_t v);
hipError_t launch_maxsim_fill64(hipStream_t s, unsigned long long* p, uint64_t n, unsigned long long v);

// The candidate pass: M[t * n_groups + g] (filled with MAXSIM_KEY_NEG_INF by the caller) is raised to the ordered key of
// every row of group g against token t.  q_bf16: [ceil(n_tokens / chunk) * chunk, ldb] bf16 rows, zero past n_tokens (the
// prepare kernel's output); slab_frag, row_norm, row_sqnorm: the fragment-major slab and its per-row arrays.
hipError_t launch_maxsim_rows(hipStream_t s, int metric, const void* slab_frag, const float* row_norm, const float* row_sqnorm,
                              const void* q_bf16, uint32_t n_tokens, uint64_t n_rows, uint32_t dim, const uint32_t* group_of_row,
                              uint32_t n_groups, uint32_t* M, MaxsimRowsInfo* info);

// U[g] = maxsim_upper over bound_for_key(M[t][g], ldb, R, q_norms[t], IN_EXTRA_MFMA); -inf for a group without a row;
// ctr[GROUPS] counts the others.  Then the 64 largest U: top[0..c) = their groups, flag[top[i]] = i (flag filled with
// MAXSIM_NO_CAND by the caller), ctr[TOP] = c.  lists: MAXSIM_TOP_LISTS * KP entries of scratch.
hipError_t launch_maxsim_upper(hipStream_t s, int metric, const uint32_t* M, uint32_t n_tokens, uint32_t n_groups, uint32_t ldb,
                               double R, const double* q_norms, double* U, Cand64* lists, uint32_t* top, uint32_t* flag,
                               uint32_t* ctr);

// Every group with U >= L: list[i] = g, flag[g] = i for the first `cap` of them; ctr[SURVIVORS] counts them all.
hipError_t launch_maxsim_survivors(hipStream_t s, const double* U, uint32_t n_groups, double L, uint32_t cap, uint32_t* list,
                                   uint32_t* flag, uint32_t* ctr);

// The reference scores of the min(*n_cand, cap) flagged groups: their member rows are listed (members: row_cap entries,
// ctr[MEMBERS] zeroed by the caller), every (member, token) pair is scored in the reference's f64 order and raises
// E[cand * n_tokens + t] (zeroed by the caller), scores[cand] = the token-order sum; ctr[NAN] is set by a NaN score.
// Nothing is scored when ctr[MEMBERS] ran past row_cap.
hipError_t launch_maxsim_score(hipStream_t s, int metric, const double* master, const double* q64, uint32_t n_tokens, uint32_t dim,
                               const uint32_t* group_of_row, uint64_t n_rows, uint32_t n_groups, const uint32_t* flag,
                               const uint32_t* n_cand, uint32_t cap, MaxsimMember* members, uint32_t row_cap,
                               unsigned long long* E, double* scores, uint32_t* ctr);

// The first min(k, *n_cand) of list[0..*n_cand) by (score desc, group key asc) -> out_keys, out_scores.  Nothing when
// *n_cand exceeds cap <= MAXSIM_CAND_CAP.
hipError_t launch_maxsim_rank(hipStream_t s, const uint32_t* list, const double* scores, const uint32_t* n_cand, uint32_t cap,
                              const unsigned long long* group_keys, uint32_t k, unsigned long long* out_keys, double* out_scores);

// The exact route, one token: scores[p] (the exact scan's) raise E1[group_of_row[p]]; then acc[g] = E1[g] for the first
// token, acc[g] + E1[g] after it, E1[g] back to 0.  acc[g] of a group without a row: MAXSIM_EMPTY_BITS.
hipError_t launch_maxsim_token(hipStream_t s, const double* scores, const uint32_t* group_of_row, uint64_t n_rows,
                               uint32_t n_groups, bool first, unsigned long long* E1, double* acc, uint32_t* ctr);

}  // namespace vl
