// deep_batch_plan.hpp -- the deep-k batch (deep_batch.hip): query batches with KFAST_MAX < k <=
// VL_DEEP_MAX_K on the MFMA pass.  Pure host arithmetic, no HIP: K', the sample and its rank, the stage schedule with the
// query stripes of each stage, the occupancy bound against the candidate capacity and the queries per sequence.
// tests/native/deep_batch_plan_test.cpp checks it on the CPU.  Nothing here decides exactness (section 34's proof reads
// only counters and thresholds); the plan decides how often a query is handed back.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace vl {

constexpr uint32_t DEEP_MAX_K = 1024;        // VL_DEEP_MAX_K
constexpr uint32_t DEEP_CAND_CAP = 16384;    // candidate entries per query: 512 x 16384 fills the buffer of 2048 x 4096
constexpr uint32_t DEEP_SEQ_QUERIES = 512;   // queries per launch sequence at that capacity
constexpr uint32_t DEEP_SELECT_MAX = 16384;  // keys k_deep_select holds in LDS
constexpr uint32_t DEEP_MIN_SAMPLE_BLOCKS = 1024;  // 32 768 rows
constexpr uint32_t DEEP_MAX_STAGES = 24;
constexpr uint32_t DEEP_RING_TARGET = 16;    // expected ring entries a wave appends per 32-row block
static_assert(DEEP_CAND_CAP <= DEEP_SELECT_MAX, "a full candidate buffer must fit the selection's LDS image");
static_assert(3 * DEEP_MAX_K <= DEEP_CAND_CAP / 2, "the unsampled first stage (half the buffer, every row kept) must hold K' rows");

struct DeepPlan {
    bool ok = false;              // false: the occupancy bound exceeds the capacity -- every query is handed back
    uint32_t kprime = 0;          // K': the rank the thresholds aim at, k <= K'
    bool sampled = false;         // false: the first stage keeps every row (T = -inf), no sampling pass
    uint32_t sample_blocks = 0;   // 32-row blocks of the sample, spread evenly over the index
    uint32_t groups = 0;          // 4 per sample block: maxima over 8 rows
    uint32_t sample_rank = 0;     // the bootstrap threshold is the sample_rank-th largest group maximum
    uint32_t n_stages = 0;
    uint32_t stage_end[DEEP_MAX_STAGES + 1] = {0};  // in 32-row blocks; stage s scans [stage_end[s], stage_end[s + 1])
    uint32_t stripes[DEEP_MAX_STAGES] = {0};        // launches of stage s, each with every stripes[s]-th query of a chunk active
    uint32_t occupancy = 0;       // bound of the expected candidate count of a query at its fullest
    uint32_t seq_queries = 0;     // queries per launch sequence: whole query chunks, at most DEEP_SEQ_QUERIES
};

#if defined(__HIPCC__)
#define VL_DEEP_HD __host__ __device__
#else
#define VL_DEEP_HD
#endif
// block `i` of `sample_blocks` -> the index's 32-row block it stands for (distinct while sample_blocks <= n_blk)
VL_DEEP_HD inline uint32_t deep_sample_block(uint32_t i, uint32_t sample_blocks, uint32_t n_blk)
{
    return (uint32_t)((uint64_t)i * n_blk / sample_blocks);
}

// launches that keep a wave's ring segment safe when a fraction p of the keys passes: a block of 32 rows x qpb queries
// appends 32 qpb p entries on average; with every A-th query active that is divided by A.  A = qpb leaves one query per
// chunk: at most 32 entries per block whatever p is, below half of the smallest ring segment (128).
inline uint32_t deep_stripes(double p, uint32_t qpb)
{
    const double per_block = 32.0 * qpb * std::min(1.0, std::max(0.0, p));
    const uint32_t a = (uint32_t)std::ceil(per_block / DEEP_RING_TARGET);
    return std::min(qpb, std::max(1u, a));
}

// rows: the index's; k: k_eff in (KFAST_MAX, DEEP_MAX_K]; cap: candidate entries per query; qpb: queries per chunk of
// k_mfma_rows (128, or 96 at stride 768); first_rows: the rows of the first stage (0 = the default, 16 samples).
inline DeepPlan deep_plan(uint64_t rows, uint32_t k, uint32_t cap, uint32_t qpb, uint64_t first_rows = 0)
{
    DeepPlan p;
    if (rows == 0 || k == 0 || qpb == 0 || rows >= 0xFFFFFFE0ull) return p;
    const uint32_t n_blk = (uint32_t)((rows + 31) / 32);
    p.seq_queries = std::max(1u, DEEP_SEQ_QUERIES / qpb) * qpb;
    p.kprime = (uint32_t)std::min<uint64_t>(3ull * k, rows);
    p.sample_blocks = std::min(n_blk, std::max(DEEP_MIN_SAMPLE_BLOCKS, p.kprime));
    p.groups = 4 * p.sample_blocks;
    const uint64_t s_rows = std::min<uint64_t>(rows, 32ull * p.sample_blocks);
    uint64_t r1 = std::min<uint64_t>(rows, first_rows ? first_rows : 16 * s_rows);
    r1 = std::min<uint64_t>(rows, (r1 + 31) / 32 * 32);
    // The K'-th best of the first stage's r1 rows is about the (K' s_rows / r1)-th best of the sample; a group maximum
    // bounds a rank only up to the number of groups, and near it the bound is loose: ranks up to half the groups are used.
    // An index too small for that (fewer than 16 K' rows) takes the unsampled schedule below: K' stays 3 k, because the
    // certificate needs the room between the k-th and the K'-th key.
    const uint32_t j0 = (uint32_t)std::max<uint64_t>(1, ((uint64_t)p.kprime * s_rows + r1 - 1) / r1);
    p.sampled = j0 <= p.groups / 2;
    double e1;  // expected entries of a query after the first stage
    double p1;  // the fraction of keys the first stage keeps
    if (p.sampled) {
        p.sample_rank = std::min(2 * j0, std::max(j0, p.groups / 2));
        // a fraction sample_rank / groups of the groups of 8 holds a key >= T
        p1 = 1.0 - std::pow(1.0 - (double)p.sample_rank / p.groups, 1.0 / 8.0);
        e1 = p1 * (double)r1;
    } else {  // no rank of the sample bounds K': keep every row of a first stage that fills half the buffer
        p.sample_blocks = p.groups = p.sample_rank = 0;
        r1 = std::min<uint64_t>(rows, std::max<uint64_t>(32, (cap / 2) / 32 * 32));
        p1 = 1.0;
        e1 = (double)r1;
    }
    uint32_t b = (uint32_t)((r1 + 31) / 32);
    p.stage_end[0] = 0;
    p.stage_end[1] = b;
    p.stripes[0] = deep_stripes(p1, qpb);
    p.n_stages = 1;
    double occ = e1;
    while (b < n_blk) {  // the rows seen double: a stage appends about K' entries to the K' the compaction left
        const uint32_t e = (p.n_stages + 1 == DEEP_MAX_STAGES) ? n_blk : (uint32_t)std::min<uint64_t>(n_blk, 2ull * b);
        const double seen = std::min<double>(32.0 * b, (double)rows);
        const double ps = std::min(1.0, p.kprime / seen);
        p.stripes[p.n_stages] = deep_stripes(ps, qpb);
        occ = std::max(occ, p.kprime + ps * 32.0 * (e - b));
        p.stage_end[++p.n_stages] = e;
        b = e;
    }
    p.occupancy = (uint32_t)std::min<double>(4.0e9, std::ceil(1.25 * occ) + 64.0);
    p.ok = p.occupancy <= cap && p.kprime >= k;
    return p;
}

}  // namespace vl
