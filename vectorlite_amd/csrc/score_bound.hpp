// score_bound.hpp -- the exactness bound of the f32 scan, for the device AND the host.
//
// bound_for_key is what the finalize kernels check their candidate lists with (kernels.hip, DESIGN.md "Exactness bound").
// A range search needs the same function on the host: it turns a score threshold into a threshold on
// scan keys once per call.  Plain C++: builds with hipcc for both sides and with a host compiler alone (the CPU tests);
// compile with -ffp-contract=off like the rest of the library.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VL_BOUND_HD __host__ __device__ __forceinline__
#else
#define VL_BOUND_HD inline
#endif

namespace vl {

// the metric codes of kernels.hpp's `Metric` (asserted equal in kernels.hip)
constexpr int BOUND_COSINE = 0, BOUND_EUCLIDEAN = 1, BOUND_MANHATTAN = 2, BOUND_DOT = 3;

// Upper bound B on the REFERENCE f64 score of any row whose f32 scan key is <= t, for in-domain data
// (finite, |v| <= 2^40, row norms 0 or >= 2^-40).  u = 2^-24, n = padded dim, R = max row norm,
// Q = |query|.  Derivation in DESIGN.md ("Exactness bound"); every u-term carries a 2x safety factor.
// `in_extra` is the additional relative input-rounding term of a lower-precision candidate filter
// (bf16 MFMA path: (2 + 2^-8) * 2^-8 per product, rigorous, no safety factor needed); 0 for the f32 scan.
template <int METRIC>
VL_BOUND_HD double bound_for_key(float t_key, uint32_t n, double R, double Q, double in_extra)
{
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double nn = (double)n;
    const double t = (double)t_key;
    if (METRIC == BOUND_COSINE) {
        if (!(Q > 0.0)) return (double)INFINITY;
        return t / Q + 2.0 * (nn + 4.0) * u + in_extra + 1e-12;
    }
    if (METRIC == BOUND_DOT) {
        return t + (2.0 * (nn + 2.0) * u + in_extra) * R * Q + 1e-12 * (1.0 + R * Q);
    }
    if (METRIC == BOUND_EUCLIDEAN && in_extra > 0.0) {
        // GEMM-form key of the MFMA path: key = 2 x.q - |x|^2 = |q|^2 - |x - q|^2 (real numbers).
        // |key32 - key| <= 2 (in_extra + (n+2)u) R Q + u R^2 + u (2 R Q + R^2); u-terms doubled.
        const double err = 2.0 * in_extra * R * Q + 4.0 * (nn + 4.0) * u * (R * Q + R * R);
        double s_lo = Q * Q - t - err;
        if (!(s_lo > 0.0)) s_lo = 0.0;
        return (1.0 / (1.0 + sqrt(s_lo) * (1.0 - 1e-12))) * (1.0 + 1e-15);
    }
    const double ts = t < 0.0 ? -t : 0.0;  // key = -sum
    double d_lo;
    if (METRIC == BOUND_EUCLIDEAN) {
        d_lo = sqrt(ts) * (1.0 - 2.0 * (nn + 2.0) * u) - 4.0 * u * (R + Q);
    } else {
        d_lo = ts * (1.0 - 2.0 * (nn + 2.0) * u) - 4.0 * u * sqrt(nn) * (R + Q);
    }
    if (!(d_lo > 0.0)) d_lo = 0.0;
    return (1.0 / (1.0 + d_lo * (1.0 - 1e-12))) * (1.0 + 1e-15);
}

// ---- the score threshold of a range search, in key space (host) ------------------------------------------------------
// f32 values from -inf to +inf as unsigned integers in ascending order (-0.0 directly below +0.0), and back.
inline uint32_t f32_to_ordered(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float ordered_to_f32(uint32_t o)
{
    const uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &b, sizeof f);
    return f;
}

// A row can be left out of a range search's candidates iff bound_for_key(key) < min_score.  The bound is a composition of
// correctly rounded monotone operations, hence weakly increasing in the key: the rows left out are those with
// key <= *tau, *tau = the LARGEST f32 (-inf .. +inf) whose bound is < min_score, found by bisection over the ordered bit
// patterns (at most 34 evaluations of the bound).  Returns false when there is no such key: every row is a candidate.
// The device tests !(key <= tau), which keeps a NaN key among the candidates.
// `in_extra`: the bound's input-rounding term of the filter whose keys are compared (0: the f32 scan).
template <int METRIC>
inline bool range_tau(uint32_t n, double R, double Q, double min_score, float* tau, double in_extra = 0.0)
{
    auto out = [&](uint32_t o) { return bound_for_key<METRIC>(ordered_to_f32(o), n, R, Q, in_extra) < min_score; };
    uint32_t lo = f32_to_ordered(-INFINITY), hi = f32_to_ordered(INFINITY);
    if (!out(lo)) return false;
    if (out(hi)) {
        *tau = INFINITY;
        return true;
    }
    while (hi - lo > 1) {  // out(lo) && !out(hi)
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (out(mid)) lo = mid;
        else hi = mid;
    }
    *tau = ordered_to_f32(lo);
    return true;
}

inline bool range_tau(int metric, uint32_t n, double R, double Q, double min_score, float* tau, double in_extra = 0.0)
{
    switch (metric) {
    case BOUND_COSINE: return range_tau<BOUND_COSINE>(n, R, Q, min_score, tau, in_extra);
    case BOUND_EUCLIDEAN: return range_tau<BOUND_EUCLIDEAN>(n, R, Q, min_score, tau, in_extra);
    case BOUND_MANHATTAN: return range_tau<BOUND_MANHATTAN>(n, R, Q, min_score, tau, in_extra);
    default: return range_tau<BOUND_DOT>(n, R, Q, min_score, tau, in_extra);
    }
}

// The same threshold for a filter that keeps `key >= thr` (the MFMA batch filter): *thr = the SMALLEST
// key that is not provably out = the f32 directly above range_tau's tau, so bound(*thr) >= min_score and
// bound(prev(*thr)) < min_score.  RANGE_KEYS_ALL: no key is provably out (a -inf threshold; cosine against a zero query)
// -- every row is a candidate and *thr is not written.  RANGE_KEYS_NONE: every key is provably out (a +inf threshold) --
// no row can qualify; *thr = +inf, which no finite key reaches.
enum RangeKeys : int { RANGE_KEYS_ALL = 0, RANGE_KEYS_FROM = 1, RANGE_KEYS_NONE = 2 };
inline RangeKeys range_key_threshold(int metric, uint32_t n, double R, double Q, double min_score, double in_extra, float* thr)
{
    float tau = 0.0f;
    if (!range_tau(metric, n, R, Q, min_score, &tau, in_extra)) return RANGE_KEYS_ALL;
    *thr = INFINITY;
    if (tau == INFINITY) return RANGE_KEYS_NONE;
    *thr = ordered_to_f32(f32_to_ordered(tau) + 1u);  // tau < +inf: the successor exists
    return RANGE_KEYS_FROM;
}

}  // namespace vl
