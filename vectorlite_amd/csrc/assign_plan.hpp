// assign_plan.hpp -- nearest-label assignment of every stored row (assign.hip): the label chunk of the
// candidate pass, the keys that are comparable ACROSS LABELS for one row, the f32 keep test of the second pass with its
// margins, and the stack of row ranges the host drives the pass over.
// Plain C++ (host and device): tests/native/assign_plan_test.cpp checks the keep test and the range plan on the CPU.
// Compile with -ffp-contract=off like the rest of the library: assign_key is one rounded multiply and one rounded add.
#pragma once

#include <stdint.h>

#include <vector>

#include "score_bound.hpp"

namespace vl {

constexpr uint32_t ASSIGN_MAX_LABELS = 4096;     // VL_ASSIGN_MAX_LABELS
constexpr uint32_t ASSIGN_BLOCK_ROWS = 32;       // rows of one wave's block: the unit of a row range
constexpr uint32_t ASSIGN_CAND_CAP = 1u << 22;   // candidate pairs of one range (64 MB at 16 bytes)
constexpr double ASSIGN_IN_EXTRA = 0.0079;       // IN_EXTRA_MFMA (mfma_scan.hpp; asserted equal in assign.hip)

// Labels per LDS buffer of the pass at a bf16 row stride.  Two buffers of this size (rows padded by 32 bytes), the labels'
// scalars and the candidate rings share the 160 KB: 2 x 64 x 1056 B at stride 512, 2 x 48 x 1568 B at stride 768.  The
// query staging pads the bf16 image to whole chunks of 128 (96 at stride 768): whole multiples of this chunk.
constexpr uint32_t assign_chunk(uint32_t ldb) { return ldb <= 512 ? 64u : 48u; }

// ---- f32 neighbours ---------------------------------------------------------------------------------------------------------
VL_BOUND_HD uint32_t assign_ord(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
VL_BOUND_HD float assign_unord(uint32_t o)
{
    const uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &b, sizeof f);
    return f;
}
// x rounded to f32 upwards / downwards (+-inf and values beyond the f32 range included; NaN stays NaN)
VL_BOUND_HD float assign_f32_up(double x)
{
    const float f = (float)x;
    return (double)f < x ? assign_unord(assign_ord(f) + 1u) : f;
}
VL_BOUND_HD float assign_f32_down(double x)
{
    const float f = (float)x;
    return (double)f > x ? assign_unord(assign_ord(f) - 1u) : f;
}

// f64 scores as unsigned integers in ascending order with -0.0 folded onto +0.0 (the ranking order of every search here);
// 0 is below every encoding
VL_BOUND_HD unsigned long long assign_score_enc(double s)
{
    s = s + 0.0;
    unsigned long long b;
    memcpy(&b, &s, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
VL_BOUND_HD double assign_score_dec(unsigned long long o)
{
    const unsigned long long b = (o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFull) : ~o;
    double s;
    memcpy(&s, &b, sizeof s);
    return s;
}

// ---- keys comparable across labels -------------------------------------------------------------------------------------------
// t = the f32 MFMA sum of bf16(x^) . bf16(q), x^ the unit row, q the label.  k_mfma_rows' keys drop what is constant per
// query; one ROW compares LABELS, so these keep the label's terms and drop |x|^2:
//   cosine     t a + b      a = fl32(1 / Q), b = 0              (x^.q / Q)
//   dot        t |x| + b    b = 0                               (x.q; the f32 value of k_mfma_rows' key)
//   Euclidean  2 t |x| + b  b = -Q^2                            (2 x.q - Q^2; 2 t |x| is k_mfma_rows' w)
// The second pass uses the same form with other b (and compares with a per-row threshold): AssignLabel::b_keep.
template <int METRIC>
VL_BOUND_HD float assign_key(float t, float row_norm, float a, float b)
{
    if (METRIC == BOUND_COSINE) return t * a + b;
    if (METRIC == BOUND_DOT) return t * row_norm + b;
    return (2.0f * t) * row_norm + b;
}

struct AssignLabel {
    float a;       // cosine: fl32(1 / Q), 0 for a zero label; 1 otherwise (not read)
    float b_seed;  // the first pass' additive term
    float b_keep;  // the second pass' additive term
};

// The second pass keeps (row, label) iff assign_key(t, |x|32, a, b_keep) >= assign_row_threshold(S, ...), S = the exact
// score of the row's seed.  CLAIM: whenever bound_for_key<METRIC>(key, n, R, Q, IN_EXTRA_MFMA) >= S for k_mfma_rows' key of the
// same t, the pair is kept.  Everything is arranged so that the f32 side needs no error analysis of its last addition:
// rounding is monotone, so from the REAL inequality  t m + b_keep >= thr64  follows  fl32(fl32(t m) + b_keep) >= fl32(thr64)
// >= f32_down(thr64), and fl32(t m) is bit for bit the product k_mfma_rows forms (dot, Euclidean).  What remains are f64
// roundings of the bound (a few 2^-53 of its largest term) and, for cosine, the two f32 roundings of t fl32(1 / Q).
//   cosine     bound = t / Q + C, C = 2 (n + 4) u + in_extra + 1e-12.  |t / Q| <= 1.01 (bf16 unit row, bf16 label), a within
//              1.001 u of 1 / Q, the product one more u: |fl32(t a) - t / Q| < 3 u; thr = f32_down(S - C - 4 u - 1e-12), b = 0.
//              A zero label has bound +inf: a = 0 and b_keep = +inf keep it for every row.
//   dot        bound = key + D, D = (2 (n + 2) u + in_extra) R Q + 1e-12 (1 + R Q); |key| <= 1.03 R Q, so its three f64
//              roundings are below 2^-50 (1.1 R Q + D): b_keep = f32_up(D + that), thr = f32_down(S).
//   Euclidean  key_e = fl32(w - |x|^2_32), bound = g(Q^2 - key_e - err), g(s) = (1 + 1e-15) / (1 + sqrt(s) (1 - 1e-12)).
//              g(s) >= S  =>  s <= T(S) = D^2 (1 + 1e-9), D as join_pair_threshold derives it.  w - |x|^2_32 is within
//              1.01 u |key_e| <= 2.1 u (R Q + R^2) of key_e, the f64 evaluation of Q^2 - key_e - err within 2^-51 of its
//              largest term.  So  w - Q^2 + E >= |x|^2_32 - T  with  E = err (1 + 1e-9) + 4 u (R Q + R^2) + 2^-48 (Q^2 + R Q +
//              R^2) + 1e-35:  b_keep = f32_up(E - Q^2),  thr = f32_down(|x|^2_32 - T - 2^-50 (|x|^2_32 + T)).
template <int METRIC>
VL_BOUND_HD AssignLabel assign_label(uint32_t n, double R, double Q)
{
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double nn = (double)n;
    AssignLabel l;
    l.a = 1.0f;
    l.b_seed = 0.0f;
    if (METRIC == BOUND_COSINE) {
        l.a = Q > 0.0 ? (float)(1.0 / Q) : 0.0f;
        l.b_keep = Q > 0.0 ? 0.0f : INFINITY;
    } else if (METRIC == BOUND_DOT) {
        const double D = (2.0 * (nn + 2.0) * u + ASSIGN_IN_EXTRA) * R * Q + 1e-12 * (1.0 + R * Q);
        l.b_keep = assign_f32_up(D + 8.881784197001252e-16 * (1.1 * R * Q + D));
    } else {
        const double err = 2.0 * ASSIGN_IN_EXTRA * R * Q + 4.0 * (nn + 4.0) * u * (R * Q + R * R);
        const double E = err * (1.0 + 1e-9) + 4.0 * u * (R * Q + R * R) + 3.552713678800501e-15 * (Q * Q + R * Q + R * R) + 1e-35;
        l.b_seed = (float)(-(Q * Q));
        l.b_keep = assign_f32_up(E - Q * Q);
    }
    return l;
}

// sqn32: the row's stored fl32(|x|^2) (Euclidean only).  A NaN S gives a NaN threshold, which no key reaches: the call fails
// on the seed's NaN flag.
template <int METRIC>
VL_BOUND_HD float assign_row_threshold(uint32_t n, double S, float sqn32)
{
    const double u = 5.9604644775390625e-08;
    if (METRIC == BOUND_COSINE) return assign_f32_down(S - (2.0 * ((double)n + 4.0) * u + ASSIGN_IN_EXTRA + 1e-12) - 4.0 * u - 1e-12);
    if (METRIC == BOUND_DOT) return assign_f32_down(S);
    if (S != S) return (float)S;
    if (!(S > 0.0)) return -INFINITY;  // every distance reaches a score <= 0
    double D = (((1.0 + 1e-15) / S - 1.0) + 1.7763568394002505e-15) * (1.0 + 1e-11) / (1.0 - 1e-12);
    if (!(D > 0.0)) D = 0.0;
    const double T = D * D * (1.0 + 1e-9);
    const double x2 = (double)sqn32;
    return assign_f32_down((x2 - T) - 8.881784197001252e-16 * (x2 + T));
}

// ---- the row ranges --------------------------------------------------------------------------------------------------------
// A range is the 32-row blocks [b0, b1).  The candidate buffer holds `cap` pairs; a range of one block cannot hold more than
// 32 n_labels, so cap is clamped to that and a single block never overflows.  The first ranges hold cap / 4 rows (a guess:
// four candidates per row; nothing was measured); a range that overflows is halved, the lower half first.
struct AssignRange {
    uint32_t b0, b1;
};
inline uint32_t assign_cap(uint32_t cap, uint32_t n_labels)
{
    const uint32_t floor = ASSIGN_BLOCK_ROWS * n_labels;
    return cap < floor ? floor : cap;
}
inline uint32_t assign_range_blocks(uint32_t cap)
{
    const uint32_t b = cap / 4u / ASSIGN_BLOCK_ROWS;
    return b < 1u ? 1u : b;
}
// the stack whose pops walk [0, n_blocks) in ascending ranges of `step` blocks
inline std::vector<AssignRange> assign_ranges(uint32_t n_blocks, uint32_t step)
{
    std::vector<AssignRange> todo;
    for (uint32_t b1 = n_blocks; b1 > 0;) {
        const uint32_t len = b1 % step ? b1 % step : step;
        todo.push_back(AssignRange{b1 - len, b1});
        b1 -= len;
    }
    return todo;
}
// an overflowed range goes back as two halves; false: it is a single block (assign_cap rules that out)
inline bool assign_split(std::vector<AssignRange>* todo, AssignRange r)
{
    if (r.b1 - r.b0 < 2) return false;
    const uint32_t mid = r.b0 + (r.b1 - r.b0) / 2;
    todo->push_back(AssignRange{mid, r.b1});
    todo->push_back(AssignRange{r.b0, mid});
    return true;
}

}  // namespace vl
