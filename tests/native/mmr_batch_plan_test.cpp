// CPU check of csrc/mmr_batch_plan.hpp: the rule that sends a batch of diversified (MMR) queries to the MFMA pass with the
// rank / similarity / selection stage or to the loop over the single diversified search.  Properties M1-M5 of the header on
// a sweep of index shapes, batch sizes, filters and sizes of S, and the named cases: the headline batch (256 queries,
// 10 M x 384, fetch_k = 20) takes the pass, two unfiltered queries and a few queries under a 1 % include token loop, an
// input that is not eligible takes the pass in no mode, and the crossovers move the right way.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../vectorlite_amd/csrc/mmr_batch_plan.hpp"

namespace {

#define CHECK(c)                                        \
    do {                                                \
        if (!(c)) {                                     \
            std::printf("FAILED %s  (line %d)\n", #c, __LINE__); \
            return 1;                                   \
        }                                               \
    } while (0)

const vl::MaskedBatchLimits LIM{8192, 2, 60, 2048};  // MFMA_MIN_ROWS, MFMA_MIN_BATCH, KFAST_MAX, a sequence at dim 384
constexpr uint64_t I8_MIN = 1024ull << 20, BF16_MIN = 512ull << 20;  // the ladder's thresholds of a new handle

enum Filter { NONE, EXCLUDE, INCLUDE };

vl::MmrBatchShape shape(uint64_t len, uint32_t dim, uint64_t m, Filter f, bool ok = true, bool rows_kernel = true)
{
    const uint32_t ldb = dim <= 128 ? 128u : dim <= 256 ? 256u : dim <= 384 ? 384u : dim <= 512 ? 512u : 768u;
    return {{ok, len, dim, (dim + 3u) & ~3u, ldb}, rows_kernel, f != NONE, f == INCLUDE, m, I8_MIN, BF16_MIN};
}

// the smallest nq in [2, 1 << 20] at which auto takes the pass (0: none)
uint64_t crossover_nq(const vl::MmrBatchShape& s)
{
    for (uint64_t nq = 2; nq <= (1u << 20); ++nq)
        if (vl::mmr_batch_route(vl::MMR_BATCH_AUTO, s, LIM, nq, 20)) return nq;
    return 0;
}

int named_cases()
{
    const uint64_t N = 10000000;
    const vl::MmrBatchShape all = shape(N, 384, N, NONE);
    // the headline: 256 queries, (4, 20) and (10, 60)
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_AUTO, all, LIM, 256, 20));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_AUTO, all, LIM, 256, 60));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_ON, all, LIM, 256, 20));
    CHECK(!vl::mmr_batch_route(vl::MMR_BATCH_OFF, all, LIM, 256, 20));
    // two unfiltered queries: two int8 passes against one sequence of the batch filter -- the loop; sixteen: the pass
    CHECK(!vl::mmr_batch_route(vl::MMR_BATCH_AUTO, all, LIM, 2, 20));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_ON, all, LIM, 2, 20));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_AUTO, all, LIM, 16, 20));
    // an exclusion token is charged like no filter at all (the masked ladder streams every row)
    CHECK(!vl::mmr_batch_route(vl::MMR_BATCH_AUTO, shape(N, 384, N - 10000, EXCLUDE), LIM, 2, 20));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_AUTO, shape(N, 384, N - 10000, EXCLUDE), LIM, 16, 20));
    // a 1 % include token: the single call reads 100 000 rows, fifteen of them cost far less than a pass over 10 M
    CHECK(!vl::mmr_batch_route(vl::MMR_BATCH_AUTO, shape(N, 384, N / 100, INCLUDE), LIM, 15, 20));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_ON, shape(N, 384, N / 100, INCLUDE), LIM, 15, 20));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_AUTO, shape(N, 384, N / 100, INCLUDE), LIM, 2048, 20));
    // a small index: the sequence's fixed tail alone outweighs the loop
    CHECK(!vl::mmr_batch_route(vl::MMR_BATCH_AUTO, shape(20000, 128, 20000, NONE), LIM, 4, 20));
    // the ladder's first stage by its own thresholds: int8 at 10 M x 384 (15 GB of f32 rows), bf16 at 512 MiB - 1 GiB, f32 below
    {
        const vl::MmrBatchShape big = shape(N, 384, N, NONE), mid = shape(400000, 384, 400000, NONE), small = shape(100000, 384, 100000, NONE);
        CHECK(vl::mmr_loop_estimate_us(big, 1) == (double)N * 384.0 / vl::MMR_LOOP_I8_BYTES_PER_US);
        CHECK(vl::mmr_loop_estimate_us(mid, 1) == 400000.0 * 384.0 * 2.0 / vl::MMR_LOOP_BF16_BYTES_PER_US);
        CHECK(vl::mmr_loop_estimate_us(small, 1) == 100000.0 * 384.0 * 4.0 / vl::MMR_LOOP_F32_BYTES_PER_US);
    }
    // not eligible: in no mode
    for (int mode = 0; mode <= 2; ++mode) {
        CHECK(!vl::mmr_batch_route(mode, shape(N, 384, N, NONE, false), LIM, 256, 20));        // forced path, Manhattan, dim 1024 ...
        CHECK(!vl::mmr_batch_route(mode, shape(8191, 384, 8191, NONE), LIM, 256, 20));         // below MFMA_MIN_ROWS
        CHECK(!vl::mmr_batch_route(mode, all, LIM, 1, 20));                                    // one query
        CHECK(!vl::mmr_batch_route(mode, all, LIM, 0, 20));
        CHECK(!vl::mmr_batch_route(mode, all, LIM, 256, 61));                                  // n beyond the list's margin
        CHECK(!vl::mmr_batch_route(mode, all, LIM, 256, 0));
        CHECK(!vl::mmr_batch_route(mode, shape(N, 384, 0, INCLUDE), LIM, 256, 20));            // an empty S
        CHECK(!vl::mmr_batch_route(mode, shape(N, 384, 5000000, EXCLUDE, true, false), LIM, 256, 20));  // a bitmap without the masked kernel
        CHECK(!vl::mmr_batch_route(mode, shape(N, 384, 5000000, INCLUDE, true, false), LIM, 256, 20));
    }
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_ON, shape(N, 384, N, NONE, true, false), LIM, 256, 20));  // no bitmap: either kernel
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_ON, all, LIM, 256, 60));
    // n = min(fetch_k, m), not fetch_k, is inside the margin: a small S is eligible at any fetch_k
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_ON, shape(N, 384, 40, INCLUDE), LIM, 2, 1024));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_ON, shape(N, 384, 60, INCLUDE), LIM, 2, 61));
    CHECK(!vl::mmr_batch_route(vl::MMR_BATCH_ON, shape(N, 384, 61, INCLUDE), LIM, 2, 61));
    // the crossovers: a handful of queries unfiltered, far more under a small include token, none for a tiny one
    const uint64_t c_all = crossover_nq(all), c_inc10 = crossover_nq(shape(N, 384, N / 10, INCLUDE)),
                   c_inc1 = crossover_nq(shape(N, 384, N / 100, INCLUDE));
    std::printf("crossover nq at 10 M x 384: %llu unfiltered, %llu include 10 %%, %llu include 1 %%\n", (unsigned long long)c_all,
                (unsigned long long)c_inc10, (unsigned long long)c_inc1);
    CHECK(c_all >= 3 && c_all <= 16);
    CHECK(c_inc10 > 2 && c_inc1 > c_inc10 && c_inc1 > 15);
    CHECK(!vl::mmr_batch_route(vl::MMR_BATCH_AUTO, all, LIM, c_all - 1, 20));
    CHECK(vl::mmr_batch_route(vl::MMR_BATCH_AUTO, all, LIM, c_all, 20));
    return 0;
}

int sweep()
{
    std::mt19937_64 rng(20241027);
    long checked = 0;
    const uint32_t dims[] = {100, 128, 256, 384, 512, 768};
    for (int it = 0; it < 20000; ++it) {
        const uint64_t len = 8192 + rng() % 20000000;
        const uint32_t dim = dims[rng() % 6];
        const uint64_t nq = 2 + rng() % 5000;
        const Filter f = (Filter)(rng() % 3);
        const uint64_t m = f == NONE ? len : 1 + rng() % len;
        const uint64_t fetch_k = 1 + rng() % 60;
        const vl::MmrBatchShape s = shape(len, dim, m, f);
        const double l0 = vl::mmr_loop_estimate_us(s, nq), p0 = vl::mmr_pass_estimate_us(s, LIM, nq);
        CHECK(l0 > 0.0 && p0 > 0.0);
        // M4
        const uint64_t nq2 = nq + 1 + rng() % 3000;
        CHECK(vl::mmr_loop_estimate_us(s, nq2) >= l0);
        CHECK(vl::mmr_pass_estimate_us(s, LIM, nq2) >= p0);
        if (f != NONE) {
            const uint64_t m2 = m + rng() % (len - m + 1);
            const vl::MmrBatchShape s2 = shape(len, dim, m2, f);
            if (f == INCLUDE) CHECK(vl::mmr_loop_estimate_us(s2, nq) >= l0);
            else CHECK(vl::mmr_loop_estimate_us(s2, nq) == l0);
            CHECK(vl::mmr_pass_estimate_us(s2, LIM, nq) == p0);
            // auto's choice is monotone in m: once the pass wins, a larger S does not lose it
            if (vl::mmr_batch_route(vl::MMR_BATCH_AUTO, s, LIM, nq, fetch_k)) CHECK(vl::mmr_batch_route(vl::MMR_BATCH_AUTO, s2, LIM, nq, fetch_k));
        }
        // M1-M3, M5
        CHECK(!vl::mmr_batch_route(vl::MMR_BATCH_OFF, s, LIM, nq, fetch_k));
        CHECK(vl::mmr_batch_route(vl::MMR_BATCH_ON, s, LIM, nq, fetch_k));
        const bool a = vl::mmr_batch_route(vl::MMR_BATCH_AUTO, s, LIM, nq, fetch_k);
        CHECK(a == (p0 < l0));
        CHECK(a == vl::mmr_batch_route(vl::MMR_BATCH_AUTO, s, LIM, nq, fetch_k));
        ++checked;
    }
    std::printf("%ld shapes checked\n", checked);
    return 0;
}

}  // namespace

int main()
{
    if (named_cases()) return 1;
    if (sweep()) return 1;
    std::printf("mmr batch plan ok\n");
    return 0;
}
