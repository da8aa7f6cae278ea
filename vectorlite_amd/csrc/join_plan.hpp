// join_plan.hpp -- how the similarity self-join's MFMA pass (join.hip) splits its triangle, and the
// key threshold it tests against.
//
// The pass computes row x row bf16 dot products for every pair of storage positions a < b.  Columns come in PANELS of `qpb`
// consecutive rows (the B operand, held in LDS), rows in BLOCKS of 32 (the A operand, streamed).  Panel y needs the blocks
// that hold a position below its last row: blocks 0 .. join_panel_blocks(y) - 1.  A UNIT is one (panel, block) pair.  Units
// are numbered panel by panel, block by block; a launch covers the panels [y0, y1) and deals the units of that range to the
// workgroups in contiguous, equally long stretches: the loads differ by at most one unit, the units of one panel are
// adjacent (a workgroup loads a panel into LDS once per stretch of it), and with the XCD rule below neighbouring stretches
// -- the same panel, or consecutive panels over the same leading blocks -- run on one XCD and share its L2.
// Plain C++ (host and device): tests/native/join_plan_test.cpp checks it on the CPU.
#pragma once

#include <stdint.h>

#include "score_bound.hpp"
#include "xcd_map.hpp"

namespace vl {

constexpr uint32_t JOIN_BLOCK_ROWS = 32;
// rows per panel at a bf16 row stride: what the LDS holds next to the candidate rings (k_mfma_rows' query chunk sizes)
constexpr uint32_t join_qpb(uint32_t ldb) { return ldb <= 512 ? 128u : 96u; }

struct JoinPlan {
    uint32_t n_rows = 0;
    uint32_t qpb = 128;       // rows per panel: a multiple of JOIN_BLOCK_ROWS
    uint32_t n_panels = 0;    // ceil(n_rows / qpb)
    uint32_t n_blocks = 0;    // ceil(n_rows / 32)
};

VL_XCD_HD inline JoinPlan join_plan(uint32_t n_rows, uint32_t qpb)
{
    JoinPlan p;
    p.n_rows = n_rows;
    p.qpb = qpb;
    p.n_panels = (n_rows + qpb - 1) / qpb;
    p.n_blocks = (n_rows + JOIN_BLOCK_ROWS - 1) / JOIN_BLOCK_ROWS;
    return p;
}

// row blocks of panel y: those with a position below the panel's last row (every full panel: (y + 1) qpb / 32)
VL_XCD_HD inline uint32_t join_panel_blocks(const JoinPlan& p, uint32_t y)
{
    const uint64_t full = (uint64_t)(y + 1) * (p.qpb / JOIN_BLOCK_ROWS);
    return full < p.n_blocks ? (uint32_t)full : p.n_blocks;
}

// units in front of panel y (y <= n_panels): only the last panel can be clipped, so the panels in front of y are full
VL_XCD_HD inline uint64_t join_units_before(const JoinPlan& p, uint32_t y)
{
    if (y == 0) return 0;
    const uint64_t q32 = p.qpb / JOIN_BLOCK_ROWS;
    const uint64_t yy = y < p.n_panels ? y : p.n_panels - 1;  // full panels in front of y
    uint64_t u = q32 * (yy * (yy + 1) / 2);
    if (y >= p.n_panels) u += join_panel_blocks(p, p.n_panels - 1);
    return u;
}

// the panel that holds unit u (u < join_units_before(n_panels)), by bisection: at most 32 steps
VL_XCD_HD inline uint32_t join_unit_panel(const JoinPlan& p, uint64_t u)
{
    uint32_t lo = 0, hi = p.n_panels;  // units_before(lo) <= u < units_before(hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (join_units_before(p, mid) <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the units [*u0, *u1) of workgroup `rank` of `n_wg` in a launch over the panels [y0, y1)
VL_XCD_HD inline void join_wg_units(const JoinPlan& p, uint32_t y0, uint32_t y1, uint32_t rank, uint32_t n_wg, uint64_t* u0,
                                    uint64_t* u1)
{
    const uint64_t b = join_units_before(p, y0), t = join_units_before(p, y1) - b;
    *u0 = b + t * rank / n_wg;
    *u1 = b + t * (rank + 1) / n_wg;
}

// The stretch a workgroup takes, from its linear id: xcd_map.hpp's rule with one column -- the workgroups of one XCD, in
// dispatch order, take consecutive stretches.
VL_XCD_HD inline uint32_t join_wg_rank(uint32_t lin, uint32_t n_wg)
{
    uint32_t x, y;
    xcd_pair(lin, n_wg, 1u, x, y);
    return x;
}

// ---- the key threshold ------------------------------------------------------------------------------------------------
// A pair's key is the f32 MFMA sum of bf16(x^_a) . bf16(x^_b), x^ = fl32(fl64(x / |x|)): batched range search's key
// (section 17) for the row a and the VIRTUAL QUERY q = fl64(x_b / |x_b|), whose staged bf16 image is row b of the slab.
// Section 17 proves score(a, q) <= bound_for_key<COSINE>(key, n, R, |q|, IN_EXTRA_MFMA).  Two steps lead from there to the
// pair's reference score, both additive and both far below this constant (derivation in DESIGN.md section 29):
//   |q| = 1 + e, |e| <= (n/2 + 3) 2^-53: the bound is evaluated at Q = 1 instead of |q|, an error of at most |key| |e|;
//   score(a, x_b) and score(a, q) are f64 evaluations of two cosines that differ by at most 2^-51 in real arithmetic, each
//   within (n + 4) 2^-52 of its real value.
// At n = 768 the three add up to less than 4.5e-13.
constexpr double JOIN_SELF_EXTRA = 1e-12;
constexpr double JOIN_IN_EXTRA = 0.0079;  // IN_EXTRA_MFMA (mfma_scan.hpp; asserted equal in join.hip)

// upper bound on the reference score of a pair whose key is <= t (weakly increasing in t, like bound_for_key)
VL_BOUND_HD double join_bound_for_key(float t, uint32_t n)
{
    return bound_for_key<BOUND_COSINE>(t, n, 1.0, 1.0, JOIN_IN_EXTRA) + JOIN_SELF_EXTRA;
}

// The smallest key that is not provably below min_score (range_key_threshold's convention and return values).  The additive
// term moves the score threshold instead of the bound: bound(t) + E >= s is tested as bound(t) >= fl(s - E), and the one
// rounding of s - E (2^-53 relative) is covered by E's factor of two over what it has to hold.
VL_BOUND_HD RangeKeys join_key_threshold(uint32_t n, double min_score, float* thr)
{
    return range_key_threshold(BOUND_COSINE, n, 1.0, 1.0, min_score - JOIN_SELF_EXTRA, JOIN_IN_EXTRA, thr);
}

// ---- Euclidean and dot: a per-pair test on the same cosine key -----------------------------------------------------------
// c = the pair's cosine key.  The real cosine of two non-zero rows is at most C(c) = c + E: join_bound_for_key's additive
// terms (the bound on the reference's f64 cosine) plus 2e-12 for that f64 cosine's own distance from the real one
// ((n + 4) 2^-52 < 1.8e-13) and for the f64 terms listed at join_pair_bound.  Derivation in DESIGN.md section 29.
VL_BOUND_HD double join_pair_extra(uint32_t n)
{
    return join_bound_for_key(0.0f, n) + 2e-12;
}

// Upper bound on the reference's f64 score of a pair with key <= c and REAL norms na, nb; weakly increasing in c (a
// composition of correctly rounded monotone steps, like bound_for_key).
//   dot:        a.b <= na nb C(c); the reference's sum is within (n + 2) 2^-52 na nb of a.b (Cauchy-Schwarz on sum |x_i y_i|).
//   Euclidean:  dist^2 >= na^2 + nb^2 - 2 na nb C(c); the reference's sum of squared differences, its sqrt and 1 / (1 + d)
//               stay inside the (1 - 1e-12) and (1 + 1e-15) factors bound_for_key<EUCLIDEAN> uses for the same steps.
template <int METRIC>
VL_BOUND_HD double join_pair_bound(float c, uint32_t n, double na, double nb)
{
    static_assert(METRIC == BOUND_DOT || METRIC == BOUND_EUCLIDEAN, "cosine has join_bound_for_key");
    const double p = na * nb;
    const double ab_hi = p > 0.0 ? ((double)c + join_pair_extra(n)) * p : 0.0;  // a zero row: a.b = 0 whatever the key
    if (METRIC == BOUND_DOT) return ab_hi + ((double)n + 2.0) * 2.220446049250313e-16 * p;
    double d2 = na * na + nb * nb - 2.0 * ab_hi;
    if (!(d2 > 0.0)) d2 = 0.0;
    return (1.0 / (1.0 + sqrt(d2) * (1.0 - 1e-12))) * (1.0 + 1e-15);
}

// x rounded to f32 upwards / downwards (+-inf and values beyond the f32 range included)
VL_BOUND_HD float join_f32_up(double x)
{
    const float f = (float)x;
    return (double)f < x ? ordered_to_f32(f32_to_ordered(f) + 1u) : f;
}
VL_BOUND_HD float join_f32_down(double x)
{
    const float f = (float)x;
    return (double)f > x ? ordered_to_f32(f32_to_ordered(f) - 1u) : f;
}

// The device works in f32 on the stored norm16 = fl32(|x|), within 1.001 u of the real norm (u = 2^-24), and forms the
// squared norms from it (3.01 u): sqnorm = fl32(|x|^2) would save 2 u of that and cost the kernel a second pair of per-row
// arrays in registers and LDS.  Its E carries 16 u more than join_pair_extra: 1.1 u for the rounding of c + E, 4.2 u for
// na32 * nb32 and the product with it, and for Euclidean 6.4 u for the squares, their sum and the final difference, which
// are relative to na^2 + nb^2 <= dist^2 + 2 na nb and so split into a relative term on dist^2 (join_pair_threshold) and
// this one.
VL_BOUND_HD float join_pair_e32(uint32_t n)
{
    return join_f32_up(join_pair_extra(n) + 16.0 * 5.9604644775390625e-08);
}

// The transformed key the kernel's epilogue compares with ONE launch scalar: a pair is a candidate iff it is >= thr.
//   dot:        an upper bound on a.b                 (c + E32) (na nb)
//   Euclidean:  minus a lower bound on dist^2         2 (c + E32) (na nb) - (na na + nb nb)
// Every operation is a single f32 rounding (2 w is exact, so a contracted 2 w - h is the same value; the translation
// units that use this are compiled with -ffp-contract=off, which keeps na na + nb nb two products and a sum).
template <int METRIC>
VL_XCD_HD inline float join_pair_key(float c, float e32, float na, float nb)
{
    if (METRIC == BOUND_COSINE) return c;
    const float w = (c + e32) * (na * nb);
    if (METRIC == BOUND_DOT) return w;
    return 2.0f * w - (na * na + nb * nb);
}

// The launch scalar for join_pair_key (dot or Euclidean), R = the largest row norm.  No pair whose join_pair_bound reaches
// min_score fails `join_pair_key >= *thr`.
//   RANGE_KEYS_ALL:  no key is provably out for the pair of largest norms (dot -inf, Euclidean min_score <= 0): not a
//                    filter's job, *thr is not written.
//   RANGE_KEYS_NONE: every key is provably out (Euclidean min_score > 1; dot > 0 over zero rows): *thr = +inf.
//   dot:        thr = min_score rounded DOWN to f32 (E32's margin leaves the transformed key above the bound itself).
//   Euclidean:  thr = -T rounded down, T = D^2 (1 + 8 u), D the largest distance whose bound reaches min_score:
//               D = ((1 + 1e-15) / min_score - 1) / (1 - 1e-12), with 2^-50 added for the rounding of the quotient and the
//               subtraction and a factor 1 + 1e-11 over the f64 steps of this function.
VL_BOUND_HD RangeKeys join_pair_threshold(int metric, uint32_t n, double R, double min_score, float* thr)
{
    const bool dot = metric == BOUND_DOT;
    auto bound = [&](float c) { return dot ? join_pair_bound<BOUND_DOT>(c, n, R, R) : join_pair_bound<BOUND_EUCLIDEAN>(c, n, R, R); };
    if (bound(-INFINITY) >= min_score) return RANGE_KEYS_ALL;
    *thr = INFINITY;
    if (!(bound(INFINITY) >= min_score)) return RANGE_KEYS_NONE;
    if (dot) {
        *thr = join_f32_down(min_score);
        return RANGE_KEYS_FROM;
    }
    const double D = (((1.0 + 1e-15) / min_score - 1.0) + 8.881784197001252e-16) * (1.0 + 1e-11) / (1.0 - 1e-12);
    *thr = -join_f32_up(D * D * (1.0 + 8.0 * 5.9604644775390625e-08));
    return RANGE_KEYS_FROM;
}

}  // namespace vl
