// The host threshold routine of a range search (csrc/score_bound.hpp, range_tau) against the host build of the SHIPPED
// bound_for_key: for every metric, over random and edge (n, R, Q, min_score),
//   bound(tau) < min_score  and  !(bound(next f32 above tau) < min_score)   (or, when there is no tau, the bound of -inf
//   already is not below min_score),
// and the bound is weakly increasing over 10^6 random adjacent f32 pairs per metric.  Host compiler, ASan + UBSan.
#include "../../vectorlite_amd/csrc/score_bound.hpp"

#include <cstdio>
#include <random>
#include <vector>

using namespace vl;

namespace {
long failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            if (++failures < 20) {        \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);      \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

template <int M>
long check_tau(uint32_t n, double R, double Q, double ms)
{
    float tau = 0.0f;
    const bool has = range_tau<M>(n, R, Q, ms, &tau);
    if (!has) {
        EXPECT(!(bound_for_key<M>(-INFINITY, n, R, Q, 0.0) < ms), "metric %d n %u R %g Q %g ms %.17g", M, n, R, Q, ms);
        return 1;
    }
    EXPECT(tau == tau, "tau is NaN");
    EXPECT(bound_for_key<M>(tau, n, R, Q, 0.0) < ms, "metric %d n %u R %g Q %g ms %.17g tau %a", M, n, R, Q, ms, (double)tau);
    if (tau != INFINITY) {
        const float up = ordered_to_f32(f32_to_ordered(tau) + 1);
        EXPECT(up > tau || (up == 0.0f && tau == 0.0f), "ordering around %a", (double)tau);
        EXPECT(!(bound_for_key<M>(up, n, R, Q, 0.0) < ms), "metric %d n %u R %g Q %g ms %.17g tau %a: the next key is out too", M,
               n, R, Q, ms, (double)tau);
    }
    return 1;
}

template <int M>
long run_metric(std::mt19937_64& rng)
{
    long checked = 0;
    const double lo_norm = 9.094947017729282e-13 /* 2^-40 */, hi_val = 1099511627776.0 /* 2^40 */;
    const uint32_t ns[] = {4, 52, 384, 768, 1000, 4096};
    std::vector<double> edge_ms = {0.0, -0.0, 1.0, 1.0000000000000002, 1.0 + 1e-9, 0.5, 1e-300, -1.0, -1e30, 1e30, INFINITY, -INFINITY};
    for (uint32_t n : ns) {
        const double hi_norm = hi_val * sqrt((double)n);
        const double Rs[] = {0.0, lo_norm, 1.0, 37.5, hi_norm};
        const double Qs[] = {0.0, lo_norm, 1.0, 19.25, hi_norm};
        for (double R : Rs)
            for (double Q : Qs) {
                for (double ms : edge_ms) checked += check_tau<M>(n, R, Q, ms);
                std::uniform_real_distribution<double> u01(0.0, 1.0);
                for (int i = 0; i < 40; ++i) {
                    double ms;
                    if (M == BOUND_DOT) ms = (u01(rng) * 2.0 - 1.0) * (R * Q + 1.0) * 1.5;
                    else if (M == BOUND_COSINE) ms = u01(rng) * 2.4 - 1.2;
                    else ms = ldexp(u01(rng), -(int)(rng() % 60));  // 1/(1+d): (0, 1], small scores included
                    checked += check_tau<M>(n, R, Q, ms);
                }
            }
    }
    // weak monotonicity over random adjacent f32 pairs (every finite key and both infinities)
    const uint32_t first = f32_to_ordered(-INFINITY), last = f32_to_ordered(INFINITY);
    for (int i = 0; i < 1000000; ++i) {
        const uint32_t o = first + (uint32_t)(rng() % (uint64_t)(last - first));
        const uint32_t n = ns[rng() % 6];
        const double R = ldexp(1.0, (int)(rng() % 60) - 30), Q = (i % 97 == 0) ? 0.0 : ldexp(1.0, (int)(rng() % 60) - 30);
        const double a = bound_for_key<M>(ordered_to_f32(o), n, R, Q, 0.0), b = bound_for_key<M>(ordered_to_f32(o + 1), n, R, Q, 0.0);
        EXPECT(a <= b, "metric %d: bound decreases between %a and its successor (%.17g > %.17g)", M, (double)ordered_to_f32(o), a, b);
    }
    return checked;
}
}  // namespace

int main()
{
    // the ordered mapping itself
    EXPECT(f32_to_ordered(-0.0f) + 1 == f32_to_ordered(0.0f), "zeros are adjacent");
    EXPECT(ordered_to_f32(f32_to_ordered(-3.5f)) == -3.5f && ordered_to_f32(f32_to_ordered(7.25f)) == 7.25f, "round trip");
    EXPECT(f32_to_ordered(-INFINITY) < f32_to_ordered(-1.0f) && f32_to_ordered(1.0f) < f32_to_ordered(INFINITY), "order");
    std::mt19937_64 rng(20261016);
    long checked = 0;
    checked += run_metric<BOUND_COSINE>(rng);
    checked += run_metric<BOUND_EUCLIDEAN>(rng);
    checked += run_metric<BOUND_MANHATTAN>(rng);
    checked += run_metric<BOUND_DOT>(rng);
    // cosine against a zero query: the bound is +inf, every row is a candidate whatever the threshold
    float tau = 0.0f;
    EXPECT(!range_tau<BOUND_COSINE>(384, 1.0, 0.0, 0.5, &tau) && !range_tau(BOUND_COSINE, 384, 1.0, 0.0, INFINITY, &tau), "Q = 0");
    if (failures) {
        printf("%ld failures\n", failures);
        return 1;
    }
    printf("range thresholds ok: %ld thresholds, 4000000 adjacent pairs\n", checked);
    return 0;
}
