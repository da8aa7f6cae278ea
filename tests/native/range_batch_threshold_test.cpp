// The key threshold of a BATCHED range search (csrc/score_bound.hpp, range_key_threshold with the MFMA filter's in_extra)
// against the host build of the shipped bound_for_key, for the three metrics the MFMA path supports:
//   1. the bound with the bf16 in_extra is weakly increasing over adjacent f32 keys (range_threshold_test.cpp's argument
//      for in_extra = 0, repeated for the term the batch uses: the filter may then compare keys with ONE threshold);
//   2. range_tau generalised with an in_extra argument returns, at in_extra = 0 (given or defaulted), the same tau bit
//      for bit as the routine it replaced, restated below as it shipped;
//   3. thr = range_key_threshold(...) is the smallest key that is not provably out: bound(thr) >= min_score and
//      bound(prev(thr)) < min_score; "every row" and "no row" are reported as such.
// Host compiler, ASan + UBSan.
#include "../../vectorlite_amd/csrc/score_bound.hpp"

#include <cstdio>
#include <random>
#include <vector>

using namespace vl;

namespace {
constexpr double IN_EXTRA = 0.0079;  // IN_EXTRA_MFMA (mfma_scan.hpp; that header needs the HIP runtime, this test does not)

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

// range_tau as it shipped before it took an in_extra argument (the bound evaluated with the literal 0.0)
template <int METRIC>
bool shipped_range_tau(uint32_t n, double R, double Q, double min_score, float* tau)
{
    auto out = [&](uint32_t o) { return bound_for_key<METRIC>(ordered_to_f32(o), n, R, Q, 0.0) < min_score; };
    uint32_t lo = f32_to_ordered(-INFINITY), hi = f32_to_ordered(INFINITY);
    if (!out(lo)) return false;
    if (out(hi)) {
        *tau = INFINITY;
        return true;
    }
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (out(mid)) lo = mid;
        else hi = mid;
    }
    *tau = ordered_to_f32(lo);
    return true;
}

uint32_t f32_bits(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return b;
}

template <int M>
void check_same_tau(uint32_t n, double R, double Q, double ms)
{
    float a = 123.0f, b = 123.0f, c = 123.0f;
    const bool ha = shipped_range_tau<M>(n, R, Q, ms, &a);
    const bool hb = range_tau<M>(n, R, Q, ms, &b);          // defaulted
    const bool hc = range_tau(M, n, R, Q, ms, &c, 0.0);     // given, through the runtime dispatch
    EXPECT(ha == hb && ha == hc, "metric %d n %u R %g Q %g ms %.17g: existence differs", M, n, R, Q, ms);
    EXPECT(f32_bits(a) == f32_bits(b) && f32_bits(a) == f32_bits(c), "metric %d n %u R %g Q %g ms %.17g: tau %a / %a / %a", M, n, R, Q,
           ms, (double)a, (double)b, (double)c);
}

template <int M>
long check_thr(uint32_t n, double R, double Q, double ms)
{
    float thr = 123.0f;
    const RangeKeys r = range_key_threshold(M, n, R, Q, ms, IN_EXTRA, &thr);
    if (r == RANGE_KEYS_ALL) {  // not even -inf is provably out
        EXPECT(!(bound_for_key<M>(-INFINITY, n, R, Q, IN_EXTRA) < ms), "metric %d n %u R %g Q %g ms %.17g: ALL", M, n, R, Q, ms);
        EXPECT(thr == 123.0f, "ALL leaves *thr alone");
        return 1;
    }
    if (r == RANGE_KEYS_NONE) {  // even +inf is provably out
        EXPECT(bound_for_key<M>(INFINITY, n, R, Q, IN_EXTRA) < ms, "metric %d n %u R %g Q %g ms %.17g: NONE", M, n, R, Q, ms);
        EXPECT(thr == INFINITY, "NONE hands the filter +inf");
        return 1;
    }
    EXPECT(thr == thr && thr > -INFINITY, "a threshold above -inf");
    EXPECT(bound_for_key<M>(thr, n, R, Q, IN_EXTRA) >= ms, "metric %d n %u R %g Q %g ms %.17g thr %a: thr itself is provably out", M, n,
           R, Q, ms, (double)thr);
    const float prev = ordered_to_f32(f32_to_ordered(thr) - 1u);
    EXPECT(bound_for_key<M>(prev, n, R, Q, IN_EXTRA) < ms, "metric %d n %u R %g Q %g ms %.17g thr %a: the key below is not out", M, n,
           R, Q, ms, (double)thr);
    return 1;
}

template <int M>
long run_metric(std::mt19937_64& rng)
{
    long checked = 0;
    const double lo_norm = 9.094947017729282e-13 /* 2^-40 */, hi_val = 1099511627776.0 /* 2^40 */;
    const uint32_t ns[] = {128, 256, 384, 512, 768};  // the bf16 row strides with an MFMA shape
    const std::vector<double> edge_ms = {0.0, -0.0, 1.0, 1.0000000000000002, 1.0 + 1e-9, 0.5, 1e-300, -1.0, -1e30, 1e30, INFINITY, -INFINITY};
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    auto random_ms = [&](double R, double Q) {
        if (M == BOUND_DOT) return (u01(rng) * 2.0 - 1.0) * (R * Q + 1.0) * 1.5;
        if (M == BOUND_COSINE) return u01(rng) * 2.4 - 1.2;
        return ldexp(u01(rng), -(int)(rng() % 60));  // 1 / (1 + d): (0, 1], small scores included
    };
    for (uint32_t n : ns) {
        const double hi_norm = hi_val * sqrt((double)n);
        const double Rs[] = {0.0, lo_norm, 1.0, 37.5, hi_norm};
        const double Qs[] = {0.0, lo_norm, 1.0, 19.25, hi_norm};
        for (double R : Rs)
            for (double Q : Qs) {
                for (double ms : edge_ms) {
                    check_same_tau<M>(n, R, Q, ms);
                    checked += check_thr<M>(n, R, Q, ms);
                }
                for (int i = 0; i < 40; ++i) {
                    const double ms = random_ms(R, Q);
                    check_same_tau<M>(n, R, Q, ms);
                    checked += check_thr<M>(n, R, Q, ms);
                }
            }
    }
    // random keys: the threshold derived from the bound OF a key admits that key and is minimal
    const uint32_t first = f32_to_ordered(-INFINITY), last = f32_to_ordered(INFINITY);
    for (int i = 0; i < 200000; ++i) {
        const uint32_t o = first + 1 + (uint32_t)(rng() % (uint64_t)(last - first - 1));  // a finite key
        const float key = ordered_to_f32(o);
        const uint32_t n = ns[rng() % 5];
        const double R = ldexp(1.0 + u01(rng), (int)(rng() % 40) - 20), Q = ldexp(1.0 + u01(rng), (int)(rng() % 40) - 20);
        const double ms = bound_for_key<M>(key, n, R, Q, IN_EXTRA);  // the key's own bound as the score threshold
        float thr = 0.0f;
        const RangeKeys r = range_key_threshold(M, n, R, Q, ms, IN_EXTRA, &thr);
        if (r == RANGE_KEYS_FROM) {
            EXPECT(f32_to_ordered(thr) <= o, "metric %d: key %a is not provably out yet thr = %a lies above it", M, (double)key, (double)thr);
            EXPECT(bound_for_key<M>(thr, n, R, Q, IN_EXTRA) >= ms, "bound(thr) >= min_score");
            EXPECT(bound_for_key<M>(ordered_to_f32(f32_to_ordered(thr) - 1u), n, R, Q, IN_EXTRA) < ms, "bound(prev(thr)) < min_score");
        } else {
            EXPECT(r == RANGE_KEYS_ALL, "a key whose bound equals min_score exists: NONE is impossible");
        }
        ++checked;
    }
    // weak monotonicity of the bf16 bound over random adjacent f32 pairs (every finite key and both infinities)
    for (int i = 0; i < 1000000; ++i) {
        const uint32_t o = first + (uint32_t)(rng() % (uint64_t)(last - first));
        const uint32_t n = ns[rng() % 5];
        const double R = ldexp(1.0, (int)(rng() % 60) - 30), Q = (i % 97 == 0) ? 0.0 : ldexp(1.0, (int)(rng() % 60) - 30);
        const double a = bound_for_key<M>(ordered_to_f32(o), n, R, Q, IN_EXTRA), b = bound_for_key<M>(ordered_to_f32(o + 1), n, R, Q, IN_EXTRA);
        EXPECT(a <= b, "metric %d: bf16 bound decreases between %a and its successor (%.17g > %.17g)", M, (double)ordered_to_f32(o), a, b);
    }
    return checked;
}
}  // namespace

int main()
{
    std::mt19937_64 rng(20261017);
    long checked = 0;
    checked += run_metric<BOUND_COSINE>(rng);
    checked += run_metric<BOUND_EUCLIDEAN>(rng);
    checked += run_metric<BOUND_DOT>(rng);
    // range_tau at in_extra = 0 for the metric the MFMA path does not serve, too: its callers must not change either
    {
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        for (int i = 0; i < 2000; ++i)
            check_same_tau<BOUND_MANHATTAN>(384, ldexp(1.0, (int)(rng() % 40) - 20), ldexp(1.0, (int)(rng() % 40) - 20),
                                            ldexp(u01(rng), -(int)(rng() % 60)));
    }
    // the corners the batch routes to the single call, and +inf
    float thr = 0.0f;
    EXPECT(range_key_threshold(BOUND_COSINE, 384, 1.0, 0.0, 0.5, IN_EXTRA, &thr) == RANGE_KEYS_ALL, "cosine, zero query");
    EXPECT(range_key_threshold(BOUND_COSINE, 384, 1.0, 1.0, -INFINITY, IN_EXTRA, &thr) == RANGE_KEYS_ALL, "-inf");
    // +inf: no finite key passes.  Euclidean scores are bounded, so every key is out; a dot or cosine key of +inf would have
    // an infinite bound, so the threshold is the key +inf itself
    EXPECT(range_key_threshold(BOUND_EUCLIDEAN, 384, 1.0, 1.0, INFINITY, IN_EXTRA, &thr) == RANGE_KEYS_NONE && thr == INFINITY, "+inf");
    thr = 0.0f;
    EXPECT(range_key_threshold(BOUND_DOT, 384, 1.0, 1.0, INFINITY, IN_EXTRA, &thr) == RANGE_KEYS_FROM && thr == INFINITY, "+inf, dot");
    if (failures) {
        printf("%ld failures\n", failures);
        return 1;
    }
    printf("range batch thresholds ok: %ld thresholds, 3000000 adjacent pairs\n", checked);
    return 0;
}
