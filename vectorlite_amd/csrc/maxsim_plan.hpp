// maxsim_plan.hpp -- the late-interaction (MaxSim) search's constants and the per-group upper bound (maxsim.hip, DESIGN.md
// section 30).  Plain C++ (host and device): tests/native/maxsim_plan_test.cpp checks the bound's sum on the CPU.
#pragma once

#include <stdint.h>

#include "score_bound.hpp"

namespace vl {

constexpr uint32_t MAXSIM_MAX_TOKENS = 128;  // VL_MAXSIM_MAX_TOKENS

// query tokens per workgroup of the candidate pass at a bf16 row stride: the chunk the prepare kernel pads the tokens to
// (mfma_scan.hip's rs_qpb, asserted equal there) -- what the LDS holds with the padded row layout
constexpr uint32_t maxsim_qpb(uint32_t ldb) { return ldb <= 512 ? 128u : 96u; }

// ---- caps: conditions on workspace bytes, not tuned numbers ---------------------------------------------------------------
// the table M[token][group] of ordered f32 keys: 256 MB (512 Ki groups at 128 tokens, 2 Mi at 32); larger tables take the
// exact route
constexpr uint64_t MAXSIM_M_BYTES = 256ull << 20;
// groups scored exactly in one round: E[candidate][token] is 8 bytes per slot, 4 MB at 128 tokens; the rank kernel's
// two LDS arrays (score, key) of this many entries are 64 KB
constexpr uint32_t MAXSIM_CAND_CAP = 4096;
// member rows of those groups: (candidate, position) pairs of 8 bytes, 8 MB
constexpr uint32_t MAXSIM_ROW_CAP = 1u << 20;

// f32 keys from -inf to +inf as unsigned integers in ascending order; f64 scores likewise (0 is below every encoding:
// the "nothing yet" value of a fetch_max slot)
constexpr uint32_t MAXSIM_KEY_NEG_INF = 0x007FFFFFu;  // f32_to_ordered(-inf)
VL_BOUND_HD uint32_t maxsim_key_enc(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
VL_BOUND_HD float maxsim_key_dec(uint32_t o)
{
    const uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &b, sizeof f);
    return f;
}
VL_BOUND_HD unsigned long long maxsim_score_enc(double s)
{
    unsigned long long b;
    memcpy(&b, &s, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
VL_BOUND_HD double maxsim_score_dec(unsigned long long o)
{
    const unsigned long long b = (o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFull) : ~o;
    double s;
    memcpy(&s, &b, sizeof s);
    return s;
}

// ---- the upper bound's sum ---------------------------------------------------------------------------------------------------
// score(g) = fl(fl(m_0 + m_1) + m_2) ... with m_t <= b_t = bound_for_key(M[t][g]).  U(g) adds the b_t in the same order, each
// first moved up by the relative e = n_tokens 2^-52: b (1 + e) for b >= 0, b (1 - e) for b < 0 (both factors are exact
// doubles for n_tokens <= 128).  In total that is e sum|b_t| >= (2 n - 1) 2^-53 sum|b_t| after the products' own roundings,
// against a rounding error of the n - 1 additions of at most (n - 1) 2^-53 (1 + e) sum|b_t|: U is at or above the REAL sum of
// the b_t, hence above every rounding of the sum of the m_t.  Every step is a correctly rounded monotone operation, so U does
// not decrease when a key -- and with it a b_t -- is raised.
VL_BOUND_HD double maxsim_term_up(double b, uint32_t n_tokens)
{
    const double e = (double)n_tokens * 2.220446049250313e-16;  // n 2^-52
    return b >= 0.0 ? b * (1.0 + e) : b * (1.0 - e);
}
// U of terms[0..n): the host form (the device kernel runs the same two lines over the table's column)
inline double maxsim_upper(const double* terms, uint32_t n_tokens)
{
    double u = maxsim_term_up(terms[0], n_tokens);
    for (uint32_t t = 1; t < n_tokens; ++t) u = u + maxsim_term_up(terms[t], n_tokens);
    return u;
}

}  // namespace vl
