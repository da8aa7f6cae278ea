// The host arithmetic of predicate filter tokens (csrc/where_plan.hpp) on the CPU: the word-aligned chunking of a
// resolution (C1, C2) and the list / masked-ladder route of a single search (W1..W6).  Stand-alone; built with
// AddressSanitizer + UBSan.
#include "../../vectorlite_amd/csrc/where_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {
int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            ++failures;                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
        }                                                   \
    } while (0)

using namespace vl;

WhereShape shape(int stage, uint64_t len = 10000000, uint32_t ld = 384, bool ok = true)
{
    return WhereShape{ok, len, ld, ld, stage, 60};
}

// the smallest m at which auto takes the ladder, len + 1 if it never does
uint64_t crossover(const WhereShape& s, uint64_t k)
{
    uint64_t lo = 1, hi = s.len + 1;
    while (lo < hi) {  // (monotone in m: W4, checked separately)
        const uint64_t mid = lo + (hi - lo) / 2;
        if (where_route_mask(WHERE_ROUTE_AUTO, s, mid, k)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
}  // namespace

int main()
{
    // C1, C2: chunks of whole words that tile [0, n) with at most WHERE_COUNTS_MAX of them
    {
        std::mt19937_64 rng(7);
        std::vector<uint64_t> ns = {1, 63, 64, 65, 1023, 1024, 1025, 4133, 1048575, 1048576, 1048577, 1100003, 10000000, 0xFFFFFFFEull};
        for (int i = 0; i < 2000; ++i) ns.push_back(1 + rng() % 0xFFFFFFFEull);
        for (uint64_t n : ns) {
            uint32_t chunk = 0;
            const uint32_t grid = where_grid_for(n, &chunk);
            EXPECT(chunk % 64 == 0 && chunk >= 1024, "n = %llu: chunk %u", (unsigned long long)n, chunk);
            EXPECT(grid >= 1 && grid <= WHERE_COUNTS_MAX, "n = %llu: grid %u", (unsigned long long)n, grid);
            EXPECT((uint64_t)grid * chunk >= n && (uint64_t)(grid - 1) * chunk < n, "n = %llu: %u chunks of %u", (unsigned long long)n, grid, chunk);
        }
        uint32_t chunk = 0;
        EXPECT(where_grid_for(1048576, &chunk) == 1024 && chunk == 1024, "the last size with 1024-row chunks");
        EXPECT(where_grid_for(1100003, &chunk) == 1012 && chunk == 1088, "ceil(1100003 / 1024) = 1075 rounds up to 1088 (%u)", chunk);
    }
    const int stages[] = {WHERE_STAGE_I8, WHERE_STAGE_BF16, WHERE_STAGE_F32};
    const uint64_t ms[] = {0, 1, 59, 60, 61, 1000, 1000000, 2499999, 2500000, 2500001, 4999999, 5000000, 5000001, 9999999, 10000000};
    const uint64_t ks[] = {1, 10, 60, 61, 1000};
    for (int st : stages)
        for (uint64_t m : ms)
            for (uint64_t k : ks)
                for (int ok = 0; ok < 2; ++ok) {
                    const WhereShape s = shape(st, 10000000, 384, ok != 0);
                    const bool elig = ok && m > 0 && (k < m ? k : m) <= 60;
                    EXPECT(where_mask_eligible(s, m, k) == elig, "eligibility: stage %d m %llu k %llu ok %d", st, (unsigned long long)m, (unsigned long long)k, ok);
                    // W1
                    EXPECT(!where_route_mask(WHERE_ROUTE_LIST, s, m, k), "W1: list never takes the ladder");
                    if (!elig)
                        for (int mode = 0; mode < 3; ++mode) EXPECT(!where_route_mask(mode, s, m, k), "W1: not eligible, mode %d", mode);
                    // W2
                    EXPECT(where_route_mask(WHERE_ROUTE_MASK, s, m, k) == elig, "W2: mask takes it whenever eligible");
                    // W3
                    EXPECT(where_route_mask(WHERE_ROUTE_AUTO, s, m, k) == (elig && where_mask_bytes(s) < where_list_bytes(s, m)),
                           "W3: auto iff the ladder's estimate is strictly lower");
                    // W5
                    if (st == WHERE_STAGE_F32) EXPECT(!where_route_mask(WHERE_ROUTE_AUTO, s, m, k), "W5: never the ladder when f32 goes first");
                    // W6
                    EXPECT(where_route_mask(WHERE_ROUTE_AUTO, s, m, k) == where_route_mask(WHERE_ROUTE_AUTO, s, m, k), "W6");
                }
    // the estimates themselves
    {
        const WhereShape i8 = shape(WHERE_STAGE_I8), b16 = shape(WHERE_STAGE_BF16), f32 = shape(WHERE_STAGE_F32);
        EXPECT(where_list_bytes(i8, 1000) == 1000ull * 384 * 4, "the list streams f32 rows");
        EXPECT(where_mask_bytes(i8) == 10000000ull * 384, "int8 first: one byte per value");
        EXPECT(where_mask_bytes(b16) == 10000000ull * 768, "bf16 first: two");
        EXPECT(where_mask_bytes(f32) == 10000000ull * 1536, "f32 first: four");
        // strictly lower: equality stays on the list
        EXPECT(!where_route_mask(WHERE_ROUTE_AUTO, i8, 2500000, 10) && where_route_mask(WHERE_ROUTE_AUTO, i8, 2500001, 10), "int8: the tie at 25 %% is the list's");
        EXPECT(!where_route_mask(WHERE_ROUTE_AUTO, b16, 5000000, 10) && where_route_mask(WHERE_ROUTE_AUTO, b16, 5000001, 10), "bf16: the tie at 50 %% is the list's");
        EXPECT(!where_route_mask(WHERE_ROUTE_AUTO, f32, 10000000, 10), "f32: even every row kept is the list's");
    }
    // W4: monotone in m, on random shapes
    {
        std::mt19937_64 rng(11);
        for (int round = 0; round < 300; ++round) {
            const uint64_t len = 1 + rng() % 50000;
            const uint32_t ld = 4 * (1 + (uint32_t)(rng() % 300));
            WhereShape s{true, len, ld, (ld + 31) / 32 * 32, stages[rng() % 3], 60};
            const uint64_t k = 1 + rng() % 60;
            bool taken = false;
            for (uint64_t m = 1; m <= len; m += 1 + len / 997) {
                const bool t = where_route_mask(WHERE_ROUTE_AUTO, s, m, k);
                EXPECT(!(taken && !t), "W4: len %llu ld %u stage %d: taken below m = %llu, not at it", (unsigned long long)len, ld, s.first_stage, (unsigned long long)m);
                taken = taken || t;
            }
        }
    }
    // the crossover at ld = 384: in (0.2, 0.3) kept under int8, in (0.45, 0.55) under bf16, none under f32
    for (uint64_t len : {100000ull, 10000000ull}) {
        const double xi = (double)crossover(shape(WHERE_STAGE_I8, len), 10) / (double)len;
        const double xb = (double)crossover(shape(WHERE_STAGE_BF16, len), 10) / (double)len;
        EXPECT(xi > 0.2 && xi < 0.3, "int8 crossover at %.4f kept", xi);
        EXPECT(xb > 0.45 && xb < 0.55, "bf16 crossover at %.4f kept", xb);
        EXPECT(crossover(shape(WHERE_STAGE_F32, len), 10) == len + 1, "f32 first: no crossover");
    }
    // the recorded pairs at 10 M x 384 (README: 10 %% kept -> the list, 50 %% kept -> the ladder, int8 first)
    EXPECT(!where_route_mask(WHERE_ROUTE_AUTO, shape(WHERE_STAGE_I8), 1000000, 10), "10 %% kept takes the list");
    EXPECT(where_route_mask(WHERE_ROUTE_AUTO, shape(WHERE_STAGE_I8), 5000000, 10), "50 %% kept takes the ladder");
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("where plan ok\n");
    return 0;
}
