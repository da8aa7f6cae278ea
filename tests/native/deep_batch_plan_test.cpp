// deep_batch_plan.hpp and gate_deep on the CPU: a stand-alone host program (tests/test_deep_batch_plan_cpu.py builds it
// with ASan + UBSan).  For every k in (60, DEEP_MAX_K] over a set of index sizes and both chunk sizes: K' >= k, the
// occupancy bound within the capacity, the stages cover every block once, the sample within the index and its groups within
// the selection's LDS image, the stripes within a chunk; gate_deep and gate_topk are never both true.
#include <cstdio>

#include "../../vectorlite_amd/csrc/batch_gate.hpp"
#include "../../vectorlite_amd/csrc/deep_batch_plan.hpp"

using namespace vl;

static long failures = 0;
#define EXPECT(cond, ...)                \
    if (!(cond)) {                       \
        if (++failures <= 20) {          \
            printf("FAIL %s: ", #cond);  \
            printf(__VA_ARGS__);         \
            printf("\n");                \
        }                                \
    }

int main()
{
    const uint64_t rows_v[] = {8192, 8192 + 17, 16383, 16384, 20000, 40000, 98304, 1000000, 10000000, 300000000};
    const uint64_t first_v[] = {0, 8192};
    long plans = 0;
    for (uint64_t rows : rows_v)
        for (uint32_t qpb : {128u, 96u})
            for (uint64_t first : first_v)
                for (uint32_t k = 61; k <= DEEP_MAX_K; ++k) {
                    const DeepPlan p = deep_plan(rows, k, DEEP_CAND_CAP, qpb, first);
                    const uint32_t n_blk = (uint32_t)((rows + 31) / 32);
                    ++plans;
                    EXPECT(p.ok && p.kprime >= k && p.kprime <= rows, "rows %llu k %u", (unsigned long long)rows, k);
                    EXPECT(p.occupancy <= DEEP_CAND_CAP, "rows %llu k %u occupancy %u", (unsigned long long)rows, k, p.occupancy);
                    EXPECT(p.n_stages >= 1 && p.n_stages <= DEEP_MAX_STAGES && p.stage_end[0] == 0 && p.stage_end[p.n_stages] == n_blk,
                           "rows %llu k %u stages %u", (unsigned long long)rows, k, p.n_stages);
                    for (uint32_t s = 0; s < p.n_stages; ++s) {
                        EXPECT(p.stage_end[s] < p.stage_end[s + 1], "rows %llu k %u stage %u", (unsigned long long)rows, k, s);
                        EXPECT(p.stripes[s] >= 1 && p.stripes[s] <= qpb, "rows %llu k %u stage %u", (unsigned long long)rows, k, s);
                    }
                    EXPECT(32ull * p.sample_blocks < rows + 32 && p.groups == 4 * p.sample_blocks && p.groups <= DEEP_SELECT_MAX,
                           "rows %llu k %u sample %u", (unsigned long long)rows, k, p.sample_blocks);
                    EXPECT(p.sampled ? (p.sample_rank >= 1 && p.sample_rank <= p.groups && p.sample_blocks >= 1) : p.sample_blocks == 0,
                           "rows %llu k %u rank %u", (unsigned long long)rows, k, p.sample_rank);
                    if (p.sampled && p.sample_blocks > 1)
                        EXPECT(deep_sample_block(p.sample_blocks - 1, p.sample_blocks, n_blk) < n_blk &&
                                   deep_sample_block(1, p.sample_blocks, n_blk) > deep_sample_block(0, p.sample_blocks, n_blk),
                               "rows %llu k %u", (unsigned long long)rows, k);
                    EXPECT(p.seq_queries % qpb == 0 && p.seq_queries <= DEEP_SEQ_QUERIES &&
                               (uint64_t)p.seq_queries * DEEP_CAND_CAP <= 2048ull * 4096, "qpb %u", qpb);
                }
    EXPECT(!deep_plan(40000, 200, 256, 128).ok, "a capacity of 256 entries holds no plan");
    // a dense stage leaves one query per chunk at most; a sparse one runs once
    EXPECT(deep_stripes(1.0, 128) == 128 && deep_stripes(1.0, 96) == 96 && deep_stripes(1.0 / 4096, 128) == 1, "stripes");

    long gates = 0;
    for (uint64_t k = 1; k <= 1100; k += (k < 70 || k > 1020) ? 1 : 37)
        for (uint64_t nq : {1ull, 2ull, 24ull})
            for (uint64_t rows : {8191ull, 8192ull, 40000ull})
                for (int bits = 0; bits < 32; ++bits) {
                    const BatchGate g{bits & 1 ? 3 : 0, bits & 2 ? 1ull : 0ull, 384, rows, nq, k, (bits & 4) != 0, !(bits & 8), !(bits & 16),
                                      {8192, 2, 60, 2048}};
                    ++gates;
                    EXPECT(!(gate_deep(g, DEEP_MAX_K) && gate_topk(g)), "k %llu both gates", (unsigned long long)k);
                    const bool want = bits == 0 && nq >= 2 && rows >= 8192 && k > 60 && k <= DEEP_MAX_K;
                    EXPECT(gate_deep(g, DEEP_MAX_K) == want, "k %llu nq %llu rows %llu bits %d", (unsigned long long)k,
                           (unsigned long long)nq, (unsigned long long)rows, bits);
                }
    printf("%ld plans and %ld gates checked, %ld failures\n", plans, gates, failures);
    return failures ? 1 : 0;
}
