// examples_plan.hpp -- search by positive and negative examples (examples.hip): its limits, the
// layout of the staged examples, the per-example map of the candidate pass and the upper bound U a row's fused key gives
// on its score.  Plain C++ (host and device): tests/native/examples_plan_test.cpp checks the map and the bound on the CPU.
#pragma once

#include <stdint.h>

#include "score_bound.hpp"

namespace vl {

constexpr uint32_t EXAMPLES_MAX_POS = 64;  // VL_EXAMPLES_MAX_POS
constexpr uint32_t EXAMPLES_MAX_NEG = 32;  // VL_EXAMPLES_MAX_NEG
constexpr uint64_t EXAMPLES_FAST_MAX_K = 64;  // the seed list's length (KP): a larger k takes the exact route

// ---- the staged examples: 16-column blocks, positives first, the negatives from a fresh block --------------------------
// every block is all positive or all negative; at most 4 + 2 = 6 blocks = 96 LDS rows: what fits at stride 768 with the
// padded row layout (96 x (1536 + 32) bytes = 150.5 KB of the 160 KB)
constexpr uint32_t EXAMPLES_MAX_BLOCKS = (EXAMPLES_MAX_POS + 15) / 16 + (EXAMPLES_MAX_NEG + 15) / 16;
constexpr uint32_t EXAMPLES_MAX_COLS = 16 * EXAMPLES_MAX_BLOCKS;
constexpr uint32_t examples_blocks(uint32_t n) { return (n + 15u) / 16u; }
// the example behind column c of the image (positives are examples 0 .. a - 1, negatives a .. a + b - 1); ~0u: padding
constexpr uint32_t examples_col_example(uint32_t c, uint32_t a, uint32_t b)
{
    return c < 16u * examples_blocks(a) ? (c < a ? c : ~0u) : (c - 16u * examples_blocks(a) < b ? a + c - 16u * examples_blocks(a) : ~0u);
}

// ---- caps: conditions on workspace bytes, not tuned numbers ---------------------------------------------------------------
// survivor rows of one call: the rank kernel holds (f, position) of every one of them in ONE workgroup's LDS, 12 bytes
// each = 96 KB of the 160 KB; in device memory the list, the scores and the two per-side maxima are 28 bytes each (224 KB)
constexpr uint32_t EXAMPLES_CAND_CAP = 8192;
constexpr int EXAMPLES_TOP_LISTS = 64;  // workgroup lists of the seed selection

// ---- the per-example map -------------------------------------------------------------------------------------------------
// The pass leaves one f32 per row and side: the maximum over the side's examples of mapped(key) = fl(fl(key * a) + c), the
// key k_mfma_rows forms for (row, example).  (a, c) puts the keys of examples of different norm Q on one scale:
//   cosine     a = fl32(1 / Q), c = 0        key ~ cos Q      -> ~ cos          (Q = 0: a = 0, every score is 0.0)
//   Euclidean  a = 1, c = -fl32(Q^2)         key ~ Q^2 - d^2  -> ~ -d^2
//   dot        a = 1, c = 0                  the key itself
// and a padding column to -inf (a = 0, c = -inf: its key is the finite sum of a zero image).
struct ExamplesMap {
    float a, c;
};
VL_BOUND_HD ExamplesMap examples_map(int metric, double Q, bool padding)
{
    if (padding) return ExamplesMap{0.0f, -INFINITY};
    if (metric == BOUND_COSINE) return ExamplesMap{Q > 0.0 ? (float)(1.0 / Q) : 0.0f, 0.0f};
    if (metric == BOUND_EUCLIDEAN) return ExamplesMap{1.0f, -(float)(Q * Q)};
    return ExamplesMap{1.0f, 0.0f};
}
VL_BOUND_HD float examples_mapped(float key, ExamplesMap m)
{
    const float p = key * m.a;  // two roundings: the library is built with -ffp-contract=off
    return p + m.c;
}

// ---- the upper bound --------------------------------------------------------------------------------------------------------
// v moved up by 2^-50 of itself: covers the rounding of the f64 sum in front of it
VL_BOUND_HD double examples_nudge_up(double v)
{
    const double e = 8.881784197001252e-16;  // 2^-50
    return v >= 0.0 ? v * (1.0 + e) : v * (1.0 - e);
}

// Upper bound on P(x) = max_i s(p_i, x) from kp = max_i mapped(key_i): for every positive i, mapped_i <= kp implies
// bound_for_key(key_i, n, R, Q_i, in_extra) <= examples_upper_p(kp, ...) (derivation per metric: DESIGN.md section 33).
// n = padded row length, R = largest row norm, q_max = largest norm among the POSITIVES, u = 2^-24.  A composition of
// correctly rounded monotone steps: weakly increasing in kp.  (The smallest norm is not needed: every term that depends on
// Q_i grows with it, and the cosine map removes Q_i altogether.)
template <int METRIC>
VL_BOUND_HD double examples_upper_p(float kp, uint32_t n, double R, double q_max, double in_extra)
{
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double nn = (double)n;
    const double t = (double)kp;
    if (METRIC == BOUND_COSINE) {
        // key / Q = mapped / ((1 + d1)(1 + d2)), |d1| <= u (the product), |d2| <= u + 2^-53 (1 / Q rounded twice)
        const double s = t >= 0.0 ? t * (1.0 + 4.0 * u) : t * (1.0 - 4.0 * u);
        return examples_nudge_up(s + (2.0 * (nn + 4.0) * u + in_extra + 3e-12));
    }
    if (METRIC == BOUND_DOT) {
        const double rq = R * q_max;
        const double c = ((2.0 * (nn + 2.0) * u + in_extra) * rq + 1e-12 * (1.0 + rq)) * (1.0 + 1e-9) + 1e-12;
        return examples_nudge_up(t + c);
    }
    // Euclidean: Q^2 - key >= -mapped (1 -+ 2u) - 2u Q^2 (the subtraction's rounding and c = fl32(Q^2)); then the bound's own
    // error term at q_max, and 1e-14 (R + Q)^2 for the f64 evaluation of either side
    const double e = (2.0 * u * q_max * q_max + 2.0 * in_extra * R * q_max + 4.0 * (nn + 4.0) * u * (R * q_max + R * R) +
                      1e-14 * (R + q_max) * (R + q_max)) * (1.0 + 1e-9);
    const double h = t < 0.0 ? (-t) * (1.0 - 2.0 * u) : (-t) * (1.0 + 2.0 * u);
    double s_lo = h - e;
    if (!(s_lo > 0.0)) s_lo = 0.0;
    return (1.0 / (1.0 + sqrt(s_lo) * (1.0 - 2e-12))) * (1.0 + 3e-15);
}

// U(x) >= f(x): without negatives f = P; with negatives f is P or -(N N) <= 0, so f <= max(P, 0)
template <int METRIC>
VL_BOUND_HD double examples_upper(float kp, bool has_neg, uint32_t n, double R, double q_max, double in_extra)
{
    const double up = examples_upper_p<METRIC>(kp, n, R, q_max, in_extra);
    return has_neg && up < 0.0 ? 0.0 : up;
}

}  // namespace vl
