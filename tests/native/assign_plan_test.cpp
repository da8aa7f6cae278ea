// csrc/assign_plan.hpp and batch_gate.hpp's gate_assign on the CPU (host compiler, ASan + UBSan):
//   1. the second pass' f32 keep test never drops a pair whose bound_for_key reaches the seed score S: for each metric, row
//      and label norms from 2^-40 to 2^40, S placed exactly where the bound of a key crosses it (and one f64 step to either
//      side, and rounded to f32), the f32 sums around the crossing are walked bit by bit;
//   2. the stack of row ranges covers every 32-row block exactly once through any pattern of splits, lower half first;
//   3. gate_assign is on for an eligible call and off for each of its terms.
#include "../../vectorlite_amd/csrc/assign_plan.hpp"
#include "../../vectorlite_amd/csrc/batch_gate.hpp"

#include <cmath>
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

// k_mfma_rows' key of the f32 sum t for a row with the stored f32 norm and squared norm
template <int METRIC>
float rows_key(float t, float nrm, float sqn)
{
    if (METRIC == BOUND_COSINE) return t;
    if (METRIC == BOUND_DOT) return t * nrm;
    return 2.0f * t * nrm - sqn;
}

template <int METRIC>
long sweep()
{
    long checked = 0, dropped = 0;
    const int exps[] = {-40, -7, 0, 9, 40};
    const double fracs[] = {-1.0, -0.5, 0.0, 0.3, 0.9, 1.0};
    for (uint32_t n : {128u, 768u})
        for (int er : exps)
            for (double rel : {1.0, 0.37})
                for (int eq : exps) {
                    const double R = std::ldexp(1.0, er), Q = std::ldexp(1.0, eq);
                    const double rn = std::max(R * rel, std::ldexp(1.0, -40));
                    const float nrm = (float)rn, sqn = (float)(rn * rn);
                    const AssignLabel lab = assign_label<METRIC>(n, std::max(R, rn), Q);
                    for (double f : fracs) {
                        const float t0 = (float)(f * Q);
                        const double B0 = bound_for_key<METRIC>(rows_key<METRIC>(t0, nrm, sqn), n, std::max(R, rn), Q, ASSIGN_IN_EXTRA);
                        const double Ss[] = {B0, std::nextafter(B0, INFINITY), std::nextafter(B0, -INFINITY), (double)(float)B0};
                        for (double S : Ss) {
                            const float thr = assign_row_threshold<METRIC>(n, S, sqn);
                            for (int d = -6; d <= 6; ++d) {
                                const float t = assign_unord(assign_ord(t0) + (uint32_t)d);
                                const double B = bound_for_key<METRIC>(rows_key<METRIC>(t, nrm, sqn), n, std::max(R, rn), Q, ASSIGN_IN_EXTRA);
                                const bool keep = assign_key<METRIC>(t, nrm, lab.a, lab.b_keep) >= thr;
                                ++checked;
                                if (!keep) ++dropped;
                                EXPECT(!(B >= S) || keep, "metric %d n %u R 2^%d x %g Q 2^%d t %a S %a bound %a thr %a", METRIC, n, er, rel,
                                       eq, t, S, B, thr);
                            }
                        }
                    }
                }
    EXPECT(dropped > 0, "metric %d: the test keeps everything", METRIC);
    return checked;
}

// the test filters: a key far below the seed's is dropped, a zero label under cosine is kept
void filters()
{
    const AssignLabel c = assign_label<BOUND_COSINE>(384, 1.0, 2.0), z = assign_label<BOUND_COSINE>(384, 1.0, 0.0);
    EXPECT(!(assign_key<BOUND_COSINE>(1.0f, 1.f, c.a, c.b_keep) >= assign_row_threshold<BOUND_COSINE>(384, 0.9, 0.f)), "cosine 0.5 vs 0.9");
    EXPECT(assign_key<BOUND_COSINE>(1.8f, 1.f, c.a, c.b_keep) >= assign_row_threshold<BOUND_COSINE>(384, 0.9, 0.f), "cosine 0.9 vs 0.9");
    EXPECT(assign_key<BOUND_COSINE>(0.0f, 1.f, z.a, z.b_keep) >= assign_row_threshold<BOUND_COSINE>(384, 0.9, 0.f), "a zero label");
    const AssignLabel d = assign_label<BOUND_DOT>(384, 2.0, 3.0);
    EXPECT(!(assign_key<BOUND_DOT>(1.0f, 2.f, d.a, d.b_keep) >= assign_row_threshold<BOUND_DOT>(384, 4.0, 0.f)), "dot 2 vs 4");
    const AssignLabel e = assign_label<BOUND_EUCLIDEAN>(384, 1.0, 1.0);  // |x| = |q| = 1: dist^2 = 2 - 2 cos
    EXPECT(!(assign_key<BOUND_EUCLIDEAN>(0.0f, 1.f, e.a, e.b_keep) >= assign_row_threshold<BOUND_EUCLIDEAN>(384, 1.0 / 1.5, 1.f)),
           "Euclidean: distance sqrt(2) vs 0.5");
    EXPECT(assign_key<BOUND_EUCLIDEAN>(0.875f, 1.f, e.a, e.b_keep) >= assign_row_threshold<BOUND_EUCLIDEAN>(384, 1.0 / 1.5, 1.f),
           "Euclidean: distance 0.5 vs 0.5");
    EXPECT(assign_score_enc(-0.0) == assign_score_enc(0.0) && assign_score_enc(-1.0) < assign_score_enc(0.0) &&
               assign_score_enc(0.0) < assign_score_enc(5e-324) && assign_score_dec(assign_score_enc(-2.5)) == -2.5,
           "the score order");
}

long ranges()
{
    std::mt19937 rng(31);
    long plans = 0;
    for (uint32_t n_blocks : {1u, 2u, 3u, 31u, 32u, 33u, 130u, 1000u})
        for (uint32_t step : {1u, 2u, 7u, 32u, 5000u}) {
            for (int overflow_in : {0, 2, 5}) {  // 0: never; else one range in `overflow_in` longer than a block overflows
                std::vector<int> seen(n_blocks, 0);
                std::vector<AssignRange> todo = assign_ranges(n_blocks, std::min(step, n_blocks));
                uint32_t done_to = 0;
                while (!todo.empty()) {
                    const AssignRange r = todo.back();
                    todo.pop_back();
                    EXPECT(r.b0 == done_to && r.b0 < r.b1 && r.b1 <= n_blocks, "range [%u, %u) after %u of %u", r.b0, r.b1, done_to, n_blocks);
                    if (overflow_in && r.b1 - r.b0 > 1 && rng() % overflow_in == 0) {
                        EXPECT(assign_split(&todo, r), "split of [%u, %u)", r.b0, r.b1);
                        continue;
                    }
                    for (uint32_t b = r.b0; b < r.b1; ++b) ++seen[b];
                    done_to = r.b1;
                }
                for (uint32_t b = 0; b < n_blocks; ++b) EXPECT(seen[b] == 1, "block %u of %u covered %d times", b, n_blocks, seen[b]);
                ++plans;
            }
        }
    std::vector<AssignRange> one;
    EXPECT(!assign_split(&one, AssignRange{4, 5}) && one.empty(), "a single block does not split");
    EXPECT(assign_cap(100, 4096) == 32u * 4096u && assign_cap(1u << 22, 17) == (1u << 22) && assign_range_blocks(1u << 22) == (1u << 15) &&
               assign_range_blocks(10) == 1,
           "the caps");
    return plans;
}

void gate()
{
    BatchGate g{};
    g.dim = 384;
    g.rows = 4133;
    g.nq = 300;
    g.scan_supported = g.rows_kernel = true;
    EXPECT(gate_assign(g, false, true, true), "an eligible call");
    EXPECT(!gate_assign(g, true, true, true), "the exact route was asked for");
    EXPECT(!gate_assign(g, false, false, true), "Manhattan / no shape");
    EXPECT(!gate_assign(g, false, true, false), "a label outside the domain");
    BatchGate h = g;
    h.forced_path = 3;
    EXPECT(!gate_assign(h, false, true, true), "a forced path");
    h = g;
    h.out_of_domain = 1;
    EXPECT(!gate_assign(h, false, true, true), "a row outside the domain");
    h = g;
    h.env_off = true;
    EXPECT(!gate_assign(h, false, true, true), "VL_MFMA=0");
    h = g;
    h.rows_kernel = false;
    EXPECT(!gate_assign(h, false, true, true), "no row-stationary slab");
    h = g;
    h.scan_supported = false;
    EXPECT(!gate_assign(h, false, true, true), "no MFMA shape");
    h = g;
    h.dim = 0;
    EXPECT(!gate_assign(h, false, true, true), "zero-length rows");
    h = g;
    h.rows = 0xFFFFFFE0ull;
    EXPECT(!gate_assign(h, false, true, true), "2^32 - 32 rows");
    h.rows = 1;
    EXPECT(gate_assign(h, false, true, true), "no row floor");
}
}  // namespace

int main()
{
    const long keys = sweep<BOUND_COSINE>() + sweep<BOUND_EUCLIDEAN>() + sweep<BOUND_DOT>();
    filters();
    const long plans = ranges();
    gate();
    printf("%ld keys checked, %ld range plans checked, %ld failures\n", keys, plans, failures);
    return failures ? 1 : 0;
}
