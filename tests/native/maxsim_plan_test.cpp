// csrc/maxsim_plan.hpp on the CPU (host compiler, ASan + UBSan): over random keys of every metric and token counts 1 .. 128,
// the helper's U -- the sum of the bound's terms as k_maxsim_upper forms it -- is at or above the same sum evaluated in long
// double, and it does not decrease when one key is raised to its f32 successor or by a large step.  The ordered encodings
// round-trip and keep the order.
#include "../../vectorlite_amd/csrc/maxsim_plan.hpp"

#include <cstdio>
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

constexpr double IN_EXTRA = 0.0079;  // IN_EXTRA_MFMA

template <int METRIC>
double term(float key, uint32_t ldb, double R, double Q)
{
    return bound_for_key<METRIC>(key, ldb, R, Q, IN_EXTRA);
}

template <int METRIC>
double upper_of(const std::vector<float>& keys, uint32_t ldb, double R, const std::vector<double>& Q, long double* exact)
{
    std::vector<double> b(keys.size());
    long double s = 0.0L;
    for (size_t t = 0; t < keys.size(); ++t) {
        b[t] = term<METRIC>(keys[t], ldb, R, Q[t]);
        s += (long double)b[t];
    }
    if (exact) *exact = s;
    return maxsim_upper(b.data(), (uint32_t)keys.size());
}

template <int METRIC>
long run(std::mt19937_64& rng)
{
    long checked = 0;
    const uint32_t strides[] = {128, 256, 384, 512, 768};
    for (uint32_t nt = 1; nt <= MAXSIM_MAX_TOKENS; ++nt) {
        for (int rep = 0; rep < 6; ++rep) {
            const uint32_t ldb = strides[rng() % 5];
            const double R = std::exp(std::uniform_real_distribution<double>(-6.0, 6.0)(rng));
            // rep 0 .. 2: keys of mixed sign and scale (the terms cancel); 3 .. 5: keys near the top of the range
            const double scale = METRIC == BOUND_COSINE ? 1.0 : R;
            std::vector<float> keys(nt);
            std::vector<double> Q(nt);
            for (uint32_t t = 0; t < nt; ++t) {
                Q[t] = std::exp(std::uniform_real_distribution<double>(-3.0, 3.0)(rng));
                const double c = rep < 3 ? std::uniform_real_distribution<double>(-1.0, 1.0)(rng)
                                         : std::uniform_real_distribution<double>(0.9, 1.0)(rng);
                keys[t] = (float)(c * scale * Q[t]);
            }
            long double exact = 0.0L;
            const double u = upper_of<METRIC>(keys, ldb, R, Q, &exact);
            EXPECT((long double)u >= exact, "metric %d tokens %u: U %.17g below the long double sum %.21Lg", METRIC, nt, u, exact);
            // raising one key never lowers U: by one f32 step, and by a tenth of the scale
            const uint32_t which = (uint32_t)(rng() % nt);
            for (int step = 0; step < 2; ++step) {
                std::vector<float> up = keys;
                up[which] = step == 0 ? maxsim_key_dec(maxsim_key_enc(keys[which]) + 1u) : keys[which] + (float)(0.1 * scale * Q[which]);
                const double u2 = upper_of<METRIC>(up, ldb, R, Q, nullptr);
                EXPECT(u2 >= u, "metric %d tokens %u: U fell from %.17g to %.17g when key %u rose", METRIC, nt, u, u2, which);
            }
            ++checked;
        }
    }
    return checked;
}
}  // namespace

int main()
{
    std::mt19937_64 rng(30);
    long checked = run<BOUND_COSINE>(rng) + run<BOUND_EUCLIDEAN>(rng) + run<BOUND_DOT>(rng);
    // the encodings: order-preserving, invertible, -inf the smallest key, 0 below every score
    const float fs[] = {-INFINITY, -3.5f, -0.0f, 0.0f, 1e-30f, 2.0f, INFINITY};
    for (int i = 0; i < 7; ++i) {
        EXPECT(maxsim_key_dec(maxsim_key_enc(fs[i])) == fs[i], "f32 round trip %d", i);
        if (i) EXPECT(maxsim_key_enc(fs[i - 1]) < maxsim_key_enc(fs[i]), "f32 order %d", i);
        const double d = fs[i];
        EXPECT(maxsim_score_dec(maxsim_score_enc(d)) == d && maxsim_score_enc(d) > 0ull, "f64 round trip %d", i);
        if (i) EXPECT(maxsim_score_enc((double)fs[i - 1]) < maxsim_score_enc(d), "f64 order %d", i);
    }
    EXPECT(maxsim_key_enc(-INFINITY) == MAXSIM_KEY_NEG_INF, "the table's initial value is -inf");
    printf("%ld sums checked, %ld failures\n", checked, failures);
    return failures ? 1 : 0;
}
