// mfma_scan.hpp -- launch interface of the bf16 MFMA batched scan (mfma_scan.hip, K4).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.hpp"

namespace vl {

constexpr int MFMA_GROUPS = 256;       // workgroups (= row groups) of the sampling pass
constexpr int MFMA_CAND_CAP = 4096;    // candidate buffer entries per query
constexpr int MFMA_MAX_BATCH = 2048;   // queries per launch sequence (scratch is sized for this: ~70 MB per workspace);
                                       // config 5's 4096 queries are two sequences: half the fixed launches of four.
                                       // Not 4096: 32 query chunks leave the sampling pass 8 workgroups per chunk = 64 groups,
                                       // and the 64th largest of 64 group maxima is far too loose a threshold (every
                                       // candidate buffer overflowed and all queries fell back: measured)
// Fewer rows than this (MFMA_GROUPS tiles of 32) leave the sampling pass with fewer than 64 groups: no
// threshold, every score a candidate, guaranteed buffer overflow -- such indexes take the f32 batch path.
constexpr uint64_t MFMA_MIN_ROWS = (uint64_t)MFMA_GROUPS * 32;
constexpr int MFMA_MIN_BATCH = 2;      // measured at N = 10 M x 384: one bf16 pass answers 2..256 queries in 1.9-2.0 ms,
                                       // the f32 batch kernel needs 2.7-2.9 ms per pass of up to 8 (it stays for Manhattan,
                                       // row lengths without an MFMA shape, and as the fallback)

// `in_extra` of the exactness bound (bound_for_key) for the two bf16 candidate filters: the relative
// input-rounding term a bf16 row (and query) adds per product on top of the f32 scan's u-terms.
// bf16 single-query filter (k_scan_bf16): bf16 row (2^-8 after the f32 step), f32 query: u_b (1 + u) + u, rounded up.
constexpr double IN_EXTRA_BF16_SINGLE = 0.00392;
// MFMA batch filter: bf16 row and bf16 query: (2 + u) u with u = 2^-8 + 2^-23 (f64 -> f32 -> bf16 double rounding), rounded up.
constexpr double IN_EXTRA_MFMA = 0.0079;
// int8 single-query filter (k_scan_i8_qarg): its keys are upper bounds of the score in real arithmetic, so the term only
// covers their f32 evaluation: 2 (n + 8) u (1 + 2 r_max) (1 + D/Q) with n = 768, u = 2^-24,
// r_max = sqrt(768) / 254, D/Q <= 2^-11 + sqrt(768) 2^-28, rounded up.  Relative to Q (cosine) and R Q (dot).
constexpr double IN_EXTRA_I8_SINGLE = 0.000113;

// bf16 slab row stride in elements: dim rounded up to the MFMA K step (16)
// Row stride of the bf16 slab in elements: the next length the MFMA kernel has a shape for (8 / 16 / 24 / 32 / 48
// K steps of 16), zero padded -- a 100- or 300-dimensional index takes the batch filter too, at the price of the
// padding; beyond 768 dimensions there is no shape and the stride is just the dimension rounded up to 16.
inline uint32_t mfma_ldb(uint32_t dim)
{
    const uint32_t shapes[] = {128u, 256u, 384u, 512u, 768u};
    for (uint32_t s : shapes)
        if (dim <= s) return s;
    return (dim + 15u) & ~15u;
}

struct MfmaScratch {
    void* q_bf16 = nullptr;     // [nq_pad_cap, ldb] bf16
    int* gmax = nullptr;        // [nq_cap, MFMA_GROUPS]
    float* thr = nullptr;       // [nq_cap]
    Cand32* cand = nullptr;     // [nq_cap, MFMA_CAND_CAP]
    uint32_t* cnt = nullptr;    // [nq_pad_cap]
    uint32_t nq_cap = 0;        // queries per launch sequence the buffers hold
    uint32_t nq_pad_cap = 0;    // ... rounded up to whole query chunks: rows of q_bf16 and cnt (the padding queries never produce candidates)
};

bool mfma_scan_supported(uint32_t dim, int metric);

// Queries one launch sequence answers for this dimension (<= MFMA_MAX_BATCH): the sampling pass must hand k_thresholds
// at least 128 groups, i.e. 16 workgroups of 8 waves per query chunk -- at most 16 co-resident chunks on 256 CUs:
// 16 x 128 queries up to stride 512, 16 x 64 at stride 768.
uint32_t mfma_sequence_queries(uint32_t dim);
// Queries already in device memory -> the staging area of a launch sequence: d_dst [nq, dim] (zeros for a query outside
// the fast-path domain), d_norms [nq], in_domain [nq] (device-visible, e.g. pinned host memory).
hipError_t launch_stage_queries(hipStream_t s, const double* d_src, uint32_t nq, uint32_t dim, double max_abs,
                                double min_norm, double* d_dst, double* d_norms, unsigned char* in_domain);

// launch_stage_queries, the bf16 conversion of the staged queries and the clearing of the candidate counters as ONE kernel,
// for a sequence the row-stationary kernel will answer.  Returns false (nothing launched) when that kernel does not apply --
// the caller then stages with launch_stage_queries and launch_mfma_candidates converts as before; true: pass
// queries_prepared = true to launch_mfma_candidates.  *err carries the launch status.
bool launch_prepare_queries(hipStream_t s, const double* d_src, uint32_t nq, uint32_t dim, double max_abs, double min_norm,
                            double* d_dst, double* d_norms, unsigned char* in_domain, const MfmaScratch& w, hipError_t* err);

// f64 master rows [n, dim] -> UNIT-NORMALISED bf16 rows [n, ldb] (x/|x| in f64 -> f32 -> bf16, round to
// nearest even), |row| and |row|^2 (f64, rounded once to f32)
hipError_t launch_rows_bf16(hipStream_t s, const double* master, uint64_t n, uint32_t dim, void* out_bf16,
                            float* out_norm, float* out_sqnorm);

// Every bf16 row stride with an MFMA shape (128 / 256 / 384 / 512 / 768) takes the row-stationary kernel k_mfma_rows, which reads a FRAGMENT-MAJOR
// bf16 slab (launch_rows_bf16_frag); VL_MFMA_KERNEL=tile keeps the LDS-tile kernel k_mfma_scan and its row-major slab.
bool mfma_rows_kernel(uint32_t dim);
// rows [row0, row0 + n) of the index (master_rows = their f64 rows) -> the fragment-major slab and the two per-row arrays,
// all three addressed from their BASE (row 0): the layout interleaves 16 neighbouring rows
hipError_t launch_rows_bf16_frag(hipStream_t s, const double* master_rows, uint64_t row0, uint64_t n, uint32_t dim,
                                 void* slab_frag_base, float* norm_base, float* sqnorm_base);

// In-place update: rewrites, from staged f64 rows [m, dim] on the device, the rows of ONE lazy copy at the distinct positions
// pos[0..m) that lie below the copy's watermark rows_done; rows at or above it are left to the next conversion.  All arrays
// are addressed from their base (row 0).  UPDATE_COPY_BF16: out_base = the row-major bf16 slab, out_a / out_b = norm16 /
// sqnorm.  UPDATE_COPY_BF16_FRAG: the fragment-major slab and the same two arrays.  UPDATE_COPY_I8: the int8 slab, out_a =
// the (s, r) pairs, out_b = |row|.  The arithmetic is the converters' own (the same row bodies).
constexpr int UPDATE_COPY_BF16 = 0, UPDATE_COPY_BF16_FRAG = 1, UPDATE_COPY_I8 = 2;
hipError_t launch_update_copies(hipStream_t s, int copy, const double* staged, const uint32_t* pos, uint32_t m, uint64_t rows_done,
                                uint32_t dim, void* out_base, float* out_a, float* out_b);

// rows per k_mfma_scan tile (its largest shape).  The bf16 slab and the two per-row arrays must be ALLOCATED in whole tiles
// (ceil(n_rows / MFMA_TILE_ROWS) * MFMA_TILE_ROWS rows): the kernel fetches a tile as one contiguous block and masks
// the rows past n_rows afterwards, whatever they hold.
constexpr uint32_t MFMA_TILE_ROWS = 64;

// nq queries (f64 [nq, dim]) against the bf16 slab: writes one sorted top-64 candidate list per query
// (out_lists[nq][64], the layout k_merge_finalize takes with n_lists = 1).
// slab_bf16: the row-major slab, or the fragment-major one when mfma_rows_kernel(dim).
// row_norm / row_sqnorm: the arrays launch_rows_bf16 / launch_rows_bf16_frag wrote (dot and Euclidean keys need them).
// q64: [nq, dim] f64 queries followed by their [nq] f64 norms (0 = answer on the exact path: no candidates are collected).
// What one launch sequence of the filter looked like (for diagnostics: bench.py ties its PMC traffic figures to it).
struct MfmaLaunchInfo {
    int ksteps = 0;        // K steps of 16 = bf16 row stride / 16 (k_mfma_rows<KSTEPS, ...>); 0 = the LDS-tile kernel ran
    int metric = 0;
    int chunks = 0;        // query chunks (gridDim.y)
    int grid_x = 0;        // workgroups per chunk of the LAST pass-1 stage
    int stages = 0;        // pass-1 launches
    int sample_blocks = 0; // 32-row blocks the sampling pass covered
};
hipError_t launch_mfma_candidates(hipStream_t s, int metric, const void* slab_bf16, const float* row_norm,
                                  const float* row_sqnorm,
                                  const double* q64, uint32_t nq, uint64_t n_rows, uint32_t dim,
                                  const MfmaScratch& w, Cand32* out_lists, MfmaLaunchInfo* info = nullptr,
                                  bool queries_prepared = false);

// launch_mfma_candidates for queries that each exclude rows: keep_of is a DEVICE table of nq
// pointers, keep_of[q] = query q's keep bitmap (bit p & 63 of word p >> 6 set iff row p qualifies, no bit at or past
// n_rows, at least ceil(n_rows / 64) words); one shared filter is nq equal pointers.  The table must be written on
// stream s before this call.  A list holds kept rows only: min(64, kept rows of q) entries unless cnt[q] overflowed.
// The row-stationary kernel only (mfma_rows_kernel(dim)); slab_frag is the fragment-major slab.
hipError_t launch_mfma_candidates_masked(hipStream_t s, int metric, const void* slab_frag, const float* row_norm,
                                         const float* row_sqnorm, const double* q64, uint32_t nq, uint64_t n_rows, uint32_t dim,
                                         const MfmaScratch& w, const unsigned long long* const* keep_of, Cand32* out_lists,
                                         MfmaLaunchInfo* info = nullptr);

// A batch of range queries: the same pass-1 kernel with thresholds that are known before the first
// launch.  w.thr[q] = the smallest key that is not provably below the query's min_score (+inf: no candidates for this
// query), written by the caller on stream s; one launch over all rows appends every row with key >= thr[q] to
// w.cand[q * cand_cap ..], w.cnt[q] counts them (above cand_cap <= MFMA_CAND_CAP: the buffer or a ring segment overflowed).
// The row-stationary kernel only (mfma_rows_kernel(dim)); slab_frag is the fragment-major slab.
hipError_t launch_mfma_range_candidates(hipStream_t s, int metric, const void* slab_frag, const float* row_norm,
                                        const float* row_sqnorm, const double* q64, uint32_t nq, uint64_t n_rows, uint32_t dim,
                                        const MfmaScratch& w, uint32_t cand_cap, MfmaLaunchInfo* info = nullptr);

// Single-query scan of the bf16 slab (the single-query candidate filter): per-workgroup top-64 lists like launch_scan.
// Two ways to hand over the query, as launch_scan: q32_host != nullptr is the f32 query rounded from the f64 one to
// nearest even and zero padded to mfma_ldb(dim) floats, copied into the kernel arguments (q64 may then be null);
// otherwise q64 is the f64 query in device memory and each lane rounds its slice itself.  Both forms produce the same
// keys.  variant_out: SCAN16_VARIANT_BASE + G * 10000 + VPL * 100 + U of the shape that ran (above every k_scan variant).
constexpr int SCAN16_QARG_FLOATS = 768;
constexpr int SCAN16_VARIANT_BASE = 1000000;
constexpr int SCAN16_BPC = 3;       // workgroups per CU, row strides up to 512 (VL_SCAN16_BPC overrides)
constexpr int SCAN16_BPC_LONG = 2;  // ... stride 768
bool scan_bf16_supported(uint32_t dim, int metric);
hipError_t launch_scan_bf16(hipStream_t s, int metric, const void* slab_bf16, const float* row_norm,
                            const float* row_sqnorm, const double* q64, uint64_t n, uint32_t dim, Cand32* partials,
                            int* grid_out, const float* q32_host = nullptr, int* variant_out = nullptr);

// Single-query scan of the int8 copy (the first stage of the single-query ladder, cosine and dot only): per-workgroup
// top-64 lists like launch_scan_bf16, keys that bound the score from above (k_scan_i8_qarg).  The rows: launch_rows_i8
// writes [n, mfma_ldb(dim)] offset-binary bytes, one (s, r) f32 pair per row (row_sr: [n][2]) and |row| in f32.
// The query always travels in the kernel arguments, as prepare_i8_query made it.
// variant_out: SCAN8_VARIANT_BASE + G * 10000 + VPL * 100 + U (above every k_scan and k_scan_bf16 variant).
constexpr int SCAN8_QARG_HALVES = 768;
constexpr int SCAN8_VARIANT_BASE = 2000000;
constexpr int SCAN8_BPC = 3;  // workgroups per CU (VL_SCAN8_BPC overrides)
// A fixed array, filled in place (no allocation on the search path).
struct I8Query {
    uint16_t h[SCAN8_QARG_HALVES];  // f16 bits of q 2^e, zero padded past dim (f16 subnormals flushed to 0)
    float inv_scale = 1.0f;   // 2^-e
    float qd = 0.0f;          // >= |q| + D
    float d = 0.0f;           // D >= |q - 2^-e q16|
};
// dim <= SCAN8_QARG_HALVES (scan_i8_supported); fills *out
void prepare_i8_query(const double* q, uint32_t dim, I8Query* out);
bool scan_i8_supported(uint32_t dim, int metric);
hipError_t launch_rows_i8(hipStream_t s, const double* master, uint64_t n, uint32_t dim, void* out_i8, float* out_sr,
                          float* out_norm);
hipError_t launch_scan_i8(hipStream_t s, int metric, const void* slab_i8, const float* row_sr, const float* row_norm,
                          const I8Query& q, uint64_t n, uint32_t dim, Cand32* partials, int* grid_out,
                          int* variant_out = nullptr);

// The two scans under an exclusion filter's keep bitmap (kernels.hpp's launch_filter_bits): the same
// lists without the rows whose bit is 0, on the same grids (sized from n).  The query in the kernel arguments, the first
// listed shape of the stride (VL_SCAN16_SHAPE / VL_SCAN8_SHAPE do not apply).  variant_out: MASK16_VARIANT_BASE /
// MASK8_VARIANT_BASE + G * 10000 + VPL * 100 + U.
constexpr int MASK16_VARIANT_BASE = 8000000;
constexpr int MASK8_VARIANT_BASE = 9000000;
hipError_t launch_scan_bf16_masked(hipStream_t s, int metric, const void* slab_bf16, const float* row_norm,
                                   const float* row_sqnorm, const unsigned long long* keep, uint64_t n, uint32_t dim,
                                   Cand32* partials, int* grid_out, const float* q32_host, int* variant_out = nullptr);
hipError_t launch_scan_i8_masked(hipStream_t s, int metric, const void* slab_i8, const float* row_sr, const float* row_norm,
                                 const unsigned long long* keep, const I8Query& q, uint64_t n, uint32_t dim, Cand32* partials,
                                 int* grid_out, int* variant_out = nullptr);

}  // namespace vl
