// csrc/examples_plan.hpp and gate_examples on the CPU (host compiler, ASan + UBSan).  Over random and edge inputs of every
// metric: the per-example map agrees with its long double restatement, U of the fused key K = max_i mapped_i is at or above
// every example's bound_for_key value (and a long double restatement of it), U is weakly increasing in K, and with negatives
// it is max(U, 0).  The column layout holds every example once in pure blocks; gate_examples decides as its condition.
#include "../../vectorlite_amd/csrc/batch_gate.hpp"

#include <algorithm>
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
constexpr long double U24 = 5.9604644775390625e-08L;

// bound_for_key's MFMA forms, restated
template <int METRIC>
long double bound_ld(float key, uint32_t n, long double R, long double Q)
{
    const long double t = key, nn = n, ie = IN_EXTRA;
    if (METRIC == BOUND_COSINE) return t / Q + 2 * (nn + 4) * U24 + ie + 1e-12L;
    if (METRIC == BOUND_DOT) return t + (2 * (nn + 2) * U24 + ie) * R * Q + 1e-12L * (1 + R * Q);
    long double s = Q * Q - t - (2 * ie * R * Q + 4 * (nn + 4) * U24 * (R * Q + R * R));
    if (!(s > 0)) s = 0;
    return (1 / (1 + sqrtl(s) * (1 - 1e-12L))) * (1 + 1e-15L);
}

float next_up(float f) { return ordered_to_f32(f32_to_ordered(f) + 1u); }

template <int METRIC>
long run(std::mt19937_64& rng)
{
    long checked = 0;
    const uint32_t strides[] = {128, 256, 384, 512, 768};
    auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
    for (int rep = 0; rep < 4000; ++rep) {
        const uint32_t a = 1 + (uint32_t)(rng() % EXAMPLES_MAX_POS), ldb = strides[rng() % 5];
        // R and the norms over the whole domain now and then (2^-40 .. 2^40), near 1 otherwise
        const double span = rep % 8 == 0 ? 27.0 : 2.0;
        const double R = std::exp(uni(-span, span));
        std::vector<double> Q(a);
        std::vector<float> key(a), mapped(a);
        double q_max = 0.0;
        float K = -INFINITY;
        for (uint32_t i = 0; i < a; ++i) {
            Q[i] = std::exp(uni(-span, span));
            q_max = Q[i] > q_max ? Q[i] : q_max;
            // keys the pass can form: |cos| <= 1.01, |x.q| <= 1.01 R Q, 0 <= d <= R + Q -- near the top of the range half the time
            const double c = rep % 2 ? uni(-1.01, 1.01) : uni(0.9, 1.01);
            const double d = (R + Q[i]) * (rep % 2 ? uni(0.0, 1.0) : uni(0.0, 0.05));
            key[i] = (float)(METRIC == BOUND_COSINE ? c * Q[i] : (METRIC == BOUND_DOT ? c * R * Q[i] : Q[i] * Q[i] - d * d));
            mapped[i] = examples_mapped(key[i], examples_map(METRIC, Q[i], false));
            const long double want = METRIC == BOUND_COSINE ? (long double)key[i] / Q[i]
                                                            : (METRIC == BOUND_DOT ? (long double)key[i] : (long double)key[i] - (long double)Q[i] * Q[i]);
            const long double scale = METRIC == BOUND_EUCLIDEAN ? fabsl((long double)key[i]) + (long double)Q[i] * Q[i] : fabsl(want);
            EXPECT(fabsl((long double)mapped[i] - want) <= 3 * U24 * scale + 1e-40L, "metric %d: mapped %.9g against %.21Lg", METRIC,
                   (double)mapped[i], want);
            K = mapped[i] > K ? mapped[i] : K;
        }
        const double U = examples_upper<METRIC>(K, false, ldb, R, q_max, IN_EXTRA);
        for (uint32_t i = 0; i < a; ++i) {  // every mapped_i <= K
            const double b = bound_for_key<METRIC>(key[i], ldb, R, Q[i], IN_EXTRA);
            EXPECT(U >= b, "metric %d: U %.17g below example %u's bound %.17g (R %.3g Q %.3g)", METRIC, U, i, b, R, Q[i]);
            EXPECT((long double)U >= bound_ld<METRIC>(key[i], ldb, R, Q[i]), "metric %d: U %.17g below the restated bound of example %u",
                   METRIC, U, i);
        }
        // weakly increasing: one f32 step, a large step either way, and across zero
        std::vector<float> ks = {K, next_up(K), K + (float)(0.1 * (fabs((double)K) + 1e-3)), K - (float)(0.1 * (fabs((double)K) + 1e-3)),
                                 -1e-30f, -0.0f, 0.0f, 1e-30f};
        std::sort(ks.begin(), ks.end(), [](float x, float y) { return f32_to_ordered(x) < f32_to_ordered(y); });
        double prev = -INFINITY;
        for (float k2 : ks) {
            const double u2 = examples_upper<METRIC>(k2, false, ldb, R, q_max, IN_EXTRA);
            EXPECT(u2 >= prev, "metric %d: U fell from %.17g to %.17g as K rose to %.9g", METRIC, prev, u2, (double)k2);
            prev = u2;
        }
        // with negatives f <= max(P, 0)
        const double un = examples_upper<METRIC>(K, true, ldb, R, q_max, IN_EXTRA);
        EXPECT(un == (U > 0.0 ? U : 0.0), "metric %d: with negatives U is %.17g, without %.17g", METRIC, un, U);
        ++checked;
    }
    // a padding column never wins; a zero cosine example maps every key to its exact score 0
    EXPECT(examples_mapped(123.0f, examples_map(METRIC, 0.0, true)) == -INFINITY, "metric %d: padding maps to -inf", METRIC);
    if (METRIC == BOUND_COSINE) {
        EXPECT(examples_mapped(0.0f, examples_map(METRIC, 0.0, false)) == 0.0f, "a zero example maps to 0");
        EXPECT(examples_upper<METRIC>(0.0f, false, 128, 1.0, 0.0, IN_EXTRA) >= 0.0, "... and U covers its score 0");
    }
    return checked;
}

void layout()
{
    for (uint32_t a = 1; a <= EXAMPLES_MAX_POS; ++a)
        for (uint32_t b = 0; b <= EXAMPLES_MAX_NEG; ++b) {
            const uint32_t cols = 16 * (examples_blocks(a) + examples_blocks(b));
            std::vector<int> seen(a + b, 0);
            bool pure = cols <= EXAMPLES_MAX_COLS;
            for (uint32_t c = 0; c < cols; ++c) {
                const uint32_t e = examples_col_example(c, a, b);
                if (e == ~0u) continue;
                if (e >= a + b) {
                    pure = false;
                    continue;
                }
                ++seen[e];
                pure = pure && ((e < a) == (c / 16 < examples_blocks(a)));  // a block is all positive or all negative
            }
            for (uint32_t e = 0; e < a + b; ++e) pure = pure && seen[e] == 1;
            EXPECT(pure, "layout of %u positives and %u negatives", a, b);
        }
}

void gate()
{
    for (uint32_t bits = 0; bits < (1u << 10); ++bits) {
        auto on = [&](int i) { return ((bits >> i) & 1u) != 0; };
        BatchGate g{};
        g.forced_path = on(0) ? 3 : 0;
        g.out_of_domain = on(1) ? 2 : 0;
        g.env_off = on(2);
        g.scan_supported = !on(3);
        g.rows_kernel = !on(4);
        g.dim = on(5) ? 0 : 384;
        g.rows = on(6) ? 0xFFFFFFE0ull : 4133;
        g.k_eff = on(7) ? 65 : 64;
        g.nq = 96;
        const bool has_pass = !on(8), in_domain = !on(9);
        EXPECT(gate_examples(g, has_pass, in_domain) == (bits == 0), "gate_examples with term bits %x", bits);
    }
}
}  // namespace

int main()
{
    std::mt19937_64 rng(33);
    const long checked = run<BOUND_COSINE>(rng) + run<BOUND_EUCLIDEAN>(rng) + run<BOUND_DOT>(rng);
    layout();
    gate();
    printf("%ld example sets checked, %ld failures\n", checked, failures);
    return failures ? 1 : 0;
}
