// CPU check of csrc/masked_batch_plan.hpp: the rule that sends a batch of exclusion-filtered queries to the mask-aware MFMA
// pass or to the jobs kernel.  Properties R1-R5 of the header on a sweep of index shapes, batch sizes and kept fractions,
// and the named cases: the headline batch (256 queries hiding 100 ids of 10 M x 384) takes the MFMA route, two queries
// that keep 0.1 % take the jobs route, an input that is not eligible takes the MFMA route in no mode.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../vectorlite_amd/csrc/masked_batch_plan.hpp"

namespace {

#define CHECK(c)                                        \
    do {                                                \
        if (!(c)) {                                     \
            std::printf("FAILED %s  (line %d)\n", #c, __LINE__); \
            return 1;                                   \
        }                                               \
    } while (0)

const vl::MaskedBatchLimits LIM{8192, 2, 60, 2048};  // MFMA_MIN_ROWS, MFMA_MIN_BATCH, KFAST_MAX, a sequence at dim 384

vl::MaskedBatchShape shape(uint64_t len, uint32_t dim, bool ok = true)
{
    const uint32_t ldb = dim <= 128 ? 128u : dim <= 256 ? 256u : dim <= 384 ? 384u : dim <= 512 ? 512u : 768u;
    return {ok, len, dim, (dim + 3u) & ~3u, ldb};
}

int named_cases()
{
    const vl::MaskedBatchShape big = shape(10000000, 384);
    // the headline: 256 queries, 100 excluded ids each
    CHECK(vl::masked_batch_route(vl::MASKED_BATCH_AUTO, big, LIM, 256, 256ull * (10000000 - 100)));
    CHECK(vl::masked_batch_route(vl::MASKED_BATCH_ON, big, LIM, 256, 256ull * (10000000 - 100)));
    CHECK(!vl::masked_batch_route(vl::MASKED_BATCH_OFF, big, LIM, 256, 256ull * (10000000 - 100)));
    // two queries keeping 0.1 %: ten thousand rows each are a few microseconds of the jobs kernel
    CHECK(!vl::masked_batch_route(vl::MASKED_BATCH_AUTO, big, LIM, 2, 2ull * 10000));
    CHECK(vl::masked_batch_route(vl::MASKED_BATCH_ON, big, LIM, 2, 2ull * 10000));
    // a small index: the sequence's fixed tail alone outweighs the jobs kernel
    CHECK(!vl::masked_batch_route(vl::MASKED_BATCH_AUTO, shape(20000, 128), LIM, 16, 16ull * 19990));
    // not eligible: in no mode
    for (int mode = 0; mode <= 2; ++mode) {
        CHECK(!vl::masked_batch_route(mode, shape(10000000, 384, false), LIM, 256, 256ull * 9999900));  // forced path, ...
        CHECK(!vl::masked_batch_route(mode, shape(8191, 384), LIM, 256, 256ull * 8000));                 // below MFMA_MIN_ROWS
        CHECK(!vl::masked_batch_route(mode, big, LIM, 1, 9999900));                                      // a batch of one
        CHECK(!vl::masked_batch_route(mode, big, LIM, 0, 0));
    }
    CHECK(!vl::masked_query_eligible(big, LIM, 0, 10));                  // nothing kept
    CHECK(!vl::masked_query_eligible(big, LIM, 9999900, 61));            // k beyond the list's margin
    CHECK(vl::masked_query_eligible(big, LIM, 3, 61));                   // min(k, m) = 3
    CHECK(vl::masked_query_eligible(big, LIM, 9999900, 60));
    CHECK(!vl::masked_query_eligible(shape(8191, 384), LIM, 8000, 10));
    CHECK(!vl::masked_query_eligible(shape(10000000, 384, false), LIM, 9999900, 10));
    return 0;
}

int sweep()
{
    std::mt19937_64 rng(20240611);
    long checked = 0;
    const uint32_t dims[] = {100, 128, 256, 384, 512, 768};
    for (int it = 0; it < 20000; ++it) {
        const uint64_t len = 8192 + rng() % 20000000;
        const uint32_t dim = dims[rng() % 6];
        const uint64_t nq = 2 + rng() % 5000;
        const uint64_t m = 1 + rng() % len;
        const vl::MaskedBatchShape s = shape(len, dim);
        const double j0 = vl::masked_jobs_estimate_us(s, nq * m), f0 = vl::masked_mfma_estimate_us(s, LIM, nq);
        CHECK(j0 >= 0.0 && f0 > 0.0);
        // R4: more rows kept, more queries, a longer index: neither estimate goes down
        CHECK(vl::masked_jobs_estimate_us(s, nq * m + 1 + rng() % len) >= j0);
        const uint64_t nq2 = nq + 1 + rng() % 3000;
        CHECK(vl::masked_jobs_estimate_us(s, nq2 * m) >= j0);
        CHECK(vl::masked_mfma_estimate_us(s, LIM, nq2) >= f0);
        const vl::MaskedBatchShape s2 = shape(len + 1 + rng() % 1000000, dim);
        CHECK(vl::masked_mfma_estimate_us(s2, LIM, nq) >= f0);
        CHECK(vl::masked_jobs_estimate_us(s2, nq * m) >= j0);  // (the same kept rows: the jobs kernel reads only those)
        // R1-R3, R5
        CHECK(!vl::masked_batch_route(vl::MASKED_BATCH_OFF, s, LIM, nq, nq * m));
        CHECK(vl::masked_batch_route(vl::MASKED_BATCH_ON, s, LIM, nq, nq * m));
        const bool a = vl::masked_batch_route(vl::MASKED_BATCH_AUTO, s, LIM, nq, nq * m);
        CHECK(a == (f0 < j0));
        CHECK(a == vl::masked_batch_route(vl::MASKED_BATCH_AUTO, s, LIM, nq, nq * m));
        // auto's choice is monotone in the kept rows: once the MFMA route wins, keeping more rows does not lose it
        if (a) CHECK(vl::masked_batch_route(vl::MASKED_BATCH_AUTO, s, LIM, nq, nq * m + rng() % len));
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
    std::printf("masked batch plan ok\n");
    return 0;
}
