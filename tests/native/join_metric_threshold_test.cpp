// csrc/join_plan.hpp's per-pair thresholds (Euclidean, dot) on the CPU (host compiler, ASan + UBSan): the score bound is
// weakly increasing over adjacent f32 keys; the launch scalar is the directed rounding of what it bounds, with ALL / NONE
// at the corners; and the device test -- join_pair_key, the kernel's own function, in f32 on norm16 = fl32(norm) -- never
// rejects a pair whose bound reaches min_score, for keys around the point where the bound crosses min_score and norms of
// mixed length on f32 values and on the midpoints between them.
#include "../../vectorlite_amd/csrc/join_plan.hpp"

#include <cstdio>
#include <random>

using namespace vl;

namespace {
long failures = 0, checked = 0;
#define EXPECT(cond, ...)                                         \
    do {                                                          \
        if (!(cond) && ++failures < 20) printf("FAIL %s: ", #cond), printf(__VA_ARGS__), printf("\n"); \
    } while (0)

template <int METRIC>
void check_metric(std::mt19937_64& rng)
{
    constexpr bool DOT = METRIC == BOUND_DOT;
    const double norms[11] = {0.0, 0x1p-40, 0.25, 0.7071067811865476, 1.0, 1.0 + 0x1p-24, 1.0 + 3 * 0x1p-24, 4.0 - 0x1p-23, 4.0, 19.6, 0x1p40};
    const double scores_e[10] = {1e-30, 1e-6, 0.01, 0.2, 0.5, 0.75, 0.9, 1.0 - 1e-10, 1.0, 1.0 + 1e-15};
    const double scores_d[10] = {-1e12, -3.0, -1e-3, 0.0, 1e-20, 0.37, 1.0, 16.0, 384.5, 1e30};
    const double(&scores)[10] = DOT ? scores_d : scores_e;
    for (uint32_t n : {128u, 384u, 768u}) {
        const float e32 = join_pair_e32(n);
        for (int i = 0; i < 100000; ++i, ++checked) {  // monotone in the key
            const uint32_t o = (uint32_t)rng();
            const float a = ordered_to_f32(o), b = ordered_to_f32(o + 1u);
            const double na = norms[rng() % 11], nb = norms[rng() % 11];
            if (a != a || b != b || o == 0xFFFFFFFFu) continue;
            EXPECT(join_pair_bound<METRIC>(a, n, na, nb) <= join_pair_bound<METRIC>(b, n, na, nb), "n %u: bound falls at %a (%g, %g)", n, (double)a, na, nb);
        }
        for (double R : {0.25, 4.0, 19.6, 0x1p40})
            for (double ms : scores) {
                float thr = 123.0f;
                EXPECT(join_pair_threshold(METRIC, n, R, ms, &thr) == RANGE_KEYS_FROM, "ms %g", ms);
                if (DOT) {  // the largest f32 <= min_score
                    EXPECT((double)thr <= ms && (double)ordered_to_f32(f32_to_ordered(thr) + 1u) > ms, "dot ms %g: thr %a", ms, (double)thr);
                } else {    // minus the smallest f32 above D^2, D the largest distance whose bound reaches ms (+ the scalar's 2^-50)
                    const double D = ((1.0 + 1e-15) / ms - 1.0) / (1.0 - 1e-12), Da = D + 1e-15;
                    EXPECT(-(double)thr >= D * D && thr <= 0.0f, "Euclidean ms %g: thr %a", ms, (double)thr);
                    EXPECT(thr == -INFINITY || (double)ordered_to_f32(f32_to_ordered(-thr) - 1u) < Da * Da * (1.0 + 1e-6), "ms %g: thr %a is loose", ms, (double)thr);
                }
                for (double na : norms)
                    for (double nb : norms)
                        for (double na_e : {na, na * (1.0 + 0x1p-25), na * (1.0 - 0x1p-26)})  // an f32 value, a midpoint, below one
                            for (double nb_e : {nb, nb * (1.0 - 0x1p-25)}) {
                                if (na > R || nb > R) continue;
                                uint32_t lo = f32_to_ordered(-1.02f), hi = f32_to_ordered(1.02f);  // the key where the bound crosses ms
                                while (hi - lo > 1) {
                                    const uint32_t mid = lo + (hi - lo) / 2;
                                    (join_pair_bound<METRIC>(ordered_to_f32(mid), n, na_e, nb_e) >= ms ? hi : lo) = mid;
                                }
                                for (int d = -3; d <= 3; ++d) {
                                    const float c = ordered_to_f32(hi + (uint32_t)d);
                                    if (!(join_pair_bound<METRIC>(c, n, na_e, nb_e) >= ms)) continue;
                                    EXPECT(join_pair_key<METRIC>(c, e32, (float)na_e, (float)nb_e) >= thr, "metric %d n %u ms %g norms %a %a key %a: rejected",
                                           METRIC, n, ms, na_e, nb_e, (double)c);
                                    ++checked;
                                }
                            }
            }
        float thr = 123.0f;  // the corners
        EXPECT(join_pair_threshold(METRIC, n, 4.0, DOT ? -INFINITY : 0.0, &thr) == RANGE_KEYS_ALL && thr == 123.0f, "every pair: the loop");
        EXPECT(join_pair_threshold(METRIC, n, DOT ? 0.0 : 4.0, DOT ? 0.5 : 1.0001, &thr) == RANGE_KEYS_NONE && thr == INFINITY, "no pair");
    }
}
}  // namespace

int main()
{
    std::mt19937_64 rng(29);
    check_metric<BOUND_EUCLIDEAN>(rng);
    check_metric<BOUND_DOT>(rng);
    printf("%ld failures, %ld checks\n", failures, checked);
    return failures != 0;
}
