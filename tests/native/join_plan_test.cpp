// csrc/join_plan.hpp on the CPU (host compiler, ASan + UBSan):
//   1. for row counts around every block and panel edge, panel sizes 128 and 96, several grids and panel ranges, the
//      workgroups' stretches -- walked exactly as k_join_rows walks them -- cover every (row block, panel) unit of the
//      triangle exactly once, every pair a < b < n lies in a covered unit, and the loads differ by at most one unit;
//      join_wg_rank is a bijection;
//   2. the join's bound is weakly increasing over adjacent f32 keys (range_batch_threshold_test.cpp's pattern), and
//      join_key_threshold returns the smallest key whose bound reaches the moved score threshold.
#include "../../vectorlite_amd/csrc/join_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

using namespace vl;

namespace {
long failures = 0;
#define EXPECT(cond, ...)                   \
    do {                                    \
        if (!(cond)) {                      \
            if (++failures < 20) {          \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);        \
                printf("\n");               \
            }                               \
        }                                   \
    } while (0)

long check_plan(uint32_t n, uint32_t qpb, uint32_t y0, uint32_t y1, uint32_t n_wg)
{
    const JoinPlan p = join_plan(n, qpb);
    std::map<std::pair<uint32_t, uint32_t>, int> seen;  // (panel, block) -> times covered
    std::vector<uint32_t> ranks;
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t lin = 0; lin < n_wg; ++lin) {
        const uint32_t rank = join_wg_rank(lin, n_wg);
        ranks.push_back(rank);
        uint64_t u, u_end;
        join_wg_units(p, y0, y1, rank, n_wg, &u, &u_end);
        lo = std::min(lo, u_end - u);
        hi = std::max(hi, u_end - u);
        if (u >= u_end) continue;
        uint32_t y = join_unit_panel(p, u);
        for (; u < u_end; ++y) {  // the kernel's walk
            EXPECT(y >= y0 && y < y1, "n %u: panel %u outside [%u, %u)", n, y, y0, y1);
            const uint32_t b0 = (uint32_t)(u - join_units_before(p, y));
            const uint32_t nb = join_panel_blocks(p, y);
            const uint32_t b1 = (uint64_t)(nb - b0) <= u_end - u ? nb : b0 + (uint32_t)(u_end - u);
            EXPECT(b0 < b1 && b1 <= nb, "n %u panel %u: stretch [%u, %u) of %u", n, y, b0, b1, nb);
            for (uint32_t b = b0; b < b1; ++b) seen[{y, b}] += 1;
            u += b1 - b0;
        }
    }
    std::sort(ranks.begin(), ranks.end());
    for (uint32_t i = 0; i < n_wg; ++i) EXPECT(ranks[i] == i, "n_wg %u: rank %u missing", n_wg, i);
    EXPECT(hi - lo <= 1, "n %u qpb %u grid %u: loads %llu .. %llu", n, qpb, n_wg, (unsigned long long)lo, (unsigned long long)hi);
    uint64_t want = 0;
    for (uint32_t y = y0; y < y1; ++y)
        for (uint32_t b = 0; b * JOIN_BLOCK_ROWS < std::min<uint64_t>(n, (uint64_t)(y + 1) * qpb); ++b) {
            ++want;
            const auto it = seen.find(std::make_pair(y, b));
            const int times = it == seen.end() ? 0 : it->second;
            EXPECT(times == 1, "n %u qpb %u grid %u: unit (%u, %u) covered %d times", n, qpb, n_wg, y, b, times);
        }
    EXPECT(seen.size() == want, "n %u: %zu units covered, %llu in the triangle", n, seen.size(), (unsigned long long)want);
    return 1;
}
}  // namespace

int main()
{
    long plans = 0;
    for (uint32_t qpb : {128u, 96u})
        for (uint32_t base : {0u, 32u, qpb, 2 * qpb, 5 * qpb, 7 * qpb + 32})
            for (int d = -1; d <= 1; ++d) {
                const int64_t n = (int64_t)base + d;
                if (n < 2) continue;
                const uint32_t np = join_plan((uint32_t)n, qpb).n_panels;
                for (uint32_t n_wg : {1u, 3u, 8u, 13u, 256u}) {
                    plans += check_plan((uint32_t)n, qpb, 0, np, n_wg);
                    if (np >= 3) {  // the halves a split range is run as
                        plans += check_plan((uint32_t)n, qpb, 0, np / 2, n_wg);
                        plans += check_plan((uint32_t)n, qpb, np / 2, np, n_wg);
                        plans += check_plan((uint32_t)n, qpb, np - 1, np, n_wg);
                    }
                }
            }
    // large counts: the unit numbers pass 2^32, the closed forms must still agree with the panel sums at the ends
    {
        const JoinPlan p = join_plan(40000000u, 128);
        uint64_t sum = 0;
        for (uint32_t y = 0; y < p.n_panels; ++y) sum += join_panel_blocks(p, y);
        EXPECT(sum == join_units_before(p, p.n_panels) && sum > (1ull << 32), "units %llu", (unsigned long long)sum);
        EXPECT(join_unit_panel(p, sum - 1) == p.n_panels - 1 && join_unit_panel(p, 0) == 0, "ends of the bisection");
    }

    // ---- the threshold: monotone bound, smallest key not provably out ----
    std::mt19937_64 rng(29);
    long pairs = 0;
    for (uint32_t n : {128u, 384u, 768u}) {
        for (int i = 0; i < 200000; ++i) {
            const uint32_t o = (uint32_t)rng();
            const float a = ordered_to_f32(o), b = ordered_to_f32(o + 1u);
            if (a != a || b != b || o == 0xFFFFFFFFu) continue;
            EXPECT(join_bound_for_key(a, n) <= join_bound_for_key(b, n), "n %u: bound falls between %a and %a", n, (double)a, (double)b);
            ++pairs;
        }
        for (double ms : {-1.0, 0.0, 0.5, 0.8, 0.99, 1.0, 1.0078, 1.1}) {
            float thr = 123.0f;
            const RangeKeys r = join_key_threshold(n, ms, &thr);
            EXPECT(r == RANGE_KEYS_FROM, "n %u ms %g: finite thresholds have a finite key threshold", n, ms);
            const double moved = ms - JOIN_SELF_EXTRA;
            const float prev = ordered_to_f32(f32_to_ordered(thr) - 1u);
            EXPECT(bound_for_key<BOUND_COSINE>(thr, n, 1.0, 1.0, JOIN_IN_EXTRA) >= moved, "n %u ms %g: thr %a is provably out", n, ms, (double)thr);
            EXPECT(bound_for_key<BOUND_COSINE>(prev, n, 1.0, 1.0, JOIN_IN_EXTRA) < moved, "n %u ms %g: prev(thr) is not out", n, ms);
            EXPECT((double)thr <= ms, "n %u ms %g: a pair whose key equals its score is kept (thr %a)", n, ms, (double)thr);
        }
        float thr = 123.0f;
        EXPECT(join_key_threshold(n, -INFINITY, &thr) == RANGE_KEYS_ALL && thr == 123.0f, "-inf: every pair");
        EXPECT(join_key_threshold(n, INFINITY, &thr) != RANGE_KEYS_ALL && thr == INFINITY, "+inf: no finite key passes");
    }
    if (failures) {
        printf("%ld failures\n", failures);
        return 1;
    }
    printf("%ld plans checked, %ld adjacent key pairs\n", plans, pairs);
    return 0;
}
