// CPU check of csrc/grouped_batch_plan.hpp: the rule that sends a batch of grouped queries to the MFMA pass with the
// rank-and-collapse stage or to the loop over the single grouped search.  Properties G1-G5 of the header on a sweep of
// index shapes, batch sizes and sizes of S, and the named cases: the headline batch (256 queries, 10 M x 384) takes the
// pass, two queries over a tiny S loop, an input that is not eligible takes the pass in no mode, and the crossover moves
// the right way with nq and m.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../vectorlite_amd/csrc/grouped_batch_plan.hpp"

namespace {

#define CHECK(c)                                        \
    do {                                                \
        if (!(c)) {                                     \
            std::printf("FAILED %s  (line %d)\n", #c, __LINE__); \
            return 1;                                   \
        }                                               \
    } while (0)

const vl::MaskedBatchLimits LIM{8192, 2, 60, 2048};  // MFMA_MIN_ROWS, MFMA_MIN_BATCH, KFAST_MAX, a sequence at dim 384

vl::GroupedBatchShape shape(uint64_t len, uint32_t dim, uint64_t m, bool bitmap, bool ok = true, bool rows_kernel = true)
{
    const uint32_t ldb = dim <= 128 ? 128u : dim <= 256 ? 256u : dim <= 384 ? 384u : dim <= 512 ? 512u : 768u;
    return {{ok, len, dim, (dim + 3u) & ~3u, ldb}, rows_kernel, bitmap, m};
}

// the smallest m in [1, len] at which auto takes the pass for nq queries (len + 1: none)
uint64_t crossover_m(uint64_t len, uint32_t dim, uint64_t nq)
{
    uint64_t lo = 1, hi = len + 1;  // the route is monotone in m (G4): bisect
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, shape(len, dim, mid, true), LIM, nq, 10)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

int named_cases()
{
    const uint64_t N = 10000000;
    const vl::GroupedBatchShape all = shape(N, 384, N, false);
    // the headline: 256 queries, every row has a group
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, all, LIM, 256, 10));
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_ON, all, LIM, 256, 10));
    CHECK(!vl::grouped_batch_route(vl::GROUPED_BATCH_OFF, all, LIM, 256, 10));
    // 60 % of the rows grouped, 16 queries: still two passes over 6 M rows per query against one shared pass
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, shape(N, 384, 6000000, true), LIM, 16, 10));
    // two queries over an S of ten thousand rows: the loop reads a few megabytes, the pass the whole index
    CHECK(!vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, shape(N, 384, 10000, true), LIM, 2, 10));
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_ON, shape(N, 384, 10000, true), LIM, 2, 10));
    // a small index: the sequence's fixed tail alone outweighs the loop
    CHECK(!vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, shape(20000, 128, 20000, false), LIM, 4, 10));
    // not eligible: in no mode
    for (int mode = 0; mode <= 2; ++mode) {
        CHECK(!vl::grouped_batch_route(mode, shape(N, 384, N, false, false), LIM, 256, 10));       // forced path, Manhattan, dim 1024 ...
        CHECK(!vl::grouped_batch_route(mode, shape(8191, 384, 8191, false), LIM, 256, 10));        // below MFMA_MIN_ROWS
        CHECK(!vl::grouped_batch_route(mode, all, LIM, 1, 10));                                    // one query
        CHECK(!vl::grouped_batch_route(mode, all, LIM, 0, 10));
        CHECK(!vl::grouped_batch_route(mode, all, LIM, 256, 61));                                  // k beyond the list's margin
        CHECK(!vl::grouped_batch_route(mode, all, LIM, 256, 0));
        CHECK(!vl::grouped_batch_route(mode, shape(N, 384, 0, true), LIM, 256, 10));               // an empty S
        CHECK(!vl::grouped_batch_route(mode, shape(N, 384, 3, true), LIM, 256, 61));               // k, not min(k, m), is tested
        CHECK(!vl::grouped_batch_route(mode, shape(N, 384, 5000000, true, true, false), LIM, 256, 10));  // a bitmap without the masked kernel
    }
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_ON, shape(N, 384, N, false, true, false), LIM, 256, 10));  // no bitmap: either kernel
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_ON, all, LIM, 256, 60));
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_ON, shape(N, 384, 40, true), LIM, 2, 10));  // an S of 40 rows is eligible
    // the crossover: more queries make the pass pay off at a smaller S; within one sequence the pass costs the same
    const uint64_t c2 = crossover_m(N, 384, 2), c16 = crossover_m(N, 384, 16), c256 = crossover_m(N, 384, 256);
    std::printf("crossover m at 10 M x 384: %llu (2 queries), %llu (16), %llu (256)\n", (unsigned long long)c2,
                (unsigned long long)c16, (unsigned long long)c256);
    CHECK(c2 <= N && c16 < c2 && c256 < c16 && c256 >= 1);
    // ... and for a fixed nq: below the crossover the loop, at and above it the pass
    CHECK(!vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, shape(N, 384, c16 - 1, true), LIM, 16, 10));
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, shape(N, 384, c16, true), LIM, 16, 10));
    CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, shape(N, 384, N, true), LIM, 16, 10));
    return 0;
}

int sweep()
{
    std::mt19937_64 rng(20241020);
    long checked = 0;
    const uint32_t dims[] = {100, 128, 256, 384, 512, 768};
    for (int it = 0; it < 20000; ++it) {
        const uint64_t len = 8192 + rng() % 20000000;
        const uint32_t dim = dims[rng() % 6];
        const uint64_t nq = 2 + rng() % 5000;
        const uint64_t m = 1 + rng() % len;
        const uint64_t k = 1 + rng() % 60;
        const vl::GroupedBatchShape s = shape(len, dim, m, m != len);
        const double l0 = vl::grouped_loop_estimate_us(s, nq), p0 = vl::grouped_pass_estimate_us(s, LIM, nq);
        CHECK(l0 > 0.0 && p0 > 0.0);
        // G4
        const uint64_t nq2 = nq + 1 + rng() % 3000;
        CHECK(vl::grouped_loop_estimate_us(s, nq2) >= l0);
        CHECK(vl::grouped_pass_estimate_us(s, LIM, nq2) >= p0);
        const uint64_t m2 = m + rng() % (len - m + 1);
        const vl::GroupedBatchShape s2 = shape(len, dim, m2, m2 != len);
        CHECK(vl::grouped_loop_estimate_us(s2, nq) >= l0);
        CHECK(vl::grouped_pass_estimate_us(s2, LIM, nq) == p0);
        // G1-G3, G5
        CHECK(!vl::grouped_batch_route(vl::GROUPED_BATCH_OFF, s, LIM, nq, k));
        CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_ON, s, LIM, nq, k));
        const bool a = vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, s, LIM, nq, k);
        CHECK(a == (p0 < l0));
        CHECK(a == vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, s, LIM, nq, k));
        // auto's choice is monotone in m: once the pass wins, a larger S does not lose it
        if (a) CHECK(vl::grouped_batch_route(vl::GROUPED_BATCH_AUTO, s2, LIM, nq, k));
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
    std::printf("grouped batch plan ok\n");
    return 0;
}
