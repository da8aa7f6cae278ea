// Audit of the batched diversified search's stage behind k_batch_rescore on inputs handed to it
// directly.  From outside (tests/test_gpu_mmr_batch.py) a query the stage hands back without need is re-answered by the
// single call and stays exact, and random rows never put a score ON the bound.  Here launch_mmr_batch of the library
// (k_mmr_batch_rank, k_mmr_batch_select) gets hand-made candidate lists, scores, master rows and query norms, and EVERY
// word of every result block -- entries in selection order, count, flags, the words it must not touch and a guard block
// behind the last query -- is compared with the host model below: the ranking and the certificate with bound_for_key from
// score_bound.hpp (the function the device uses), the similarities as sums by index with separately rounded multiplies
// and adds (this file is built with -ffp-contract=off), the selection as the contract states it.
// Links against the built library; no other process, one pass, seconds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../vectorlite_amd/csrc/kernels.hpp"
#include "../../vectorlite_amd/csrc/mfma_scan.hpp"
#include "../../vectorlite_amd/csrc/score_bound.hpp"

namespace {

#define HIP_OK(x)                                                                                  \
    do {                                                                                           \
        const hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                                    \
            std::printf("HIP error %s at line %d: %s\n", hipGetErrorString(e_), __LINE__, #x);     \
            std::exit(2);                                                                          \
        }                                                                                          \
    } while (0)

using vl::Cand32;
using vl::KP;
using vl::SearchResultBlock;

constexpr uint32_t FILL = 0xA5A5A5A5u;
constexpr int SLOTS = 80;  // storage positions reserved per query: its 64 candidates are drawn from them

double bound(int metric, float key, uint32_t ld, double R, double Q, double in_extra)
{
    switch (metric) {
    case vl::COSINE: return vl::bound_for_key<vl::BOUND_COSINE>(key, ld, R, Q, in_extra);
    case vl::EUCLIDEAN: return vl::bound_for_key<vl::BOUND_EUCLIDEAN>(key, ld, R, Q, in_extra);
    default: return vl::bound_for_key<vl::BOUND_DOT>(key, ld, R, Q, in_extra);
    }
}

// SimilarityMetric::calculate, sums by index, every multiply and add rounded on its own
double calculate(int metric, const double* x, const double* y, uint32_t dim)
{
    if (metric == vl::COSINE) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (uint32_t i = 0; i < dim; ++i) {
            a += x[i] * y[i];
            b += x[i] * x[i];
            c += y[i] * y[i];
        }
        const double na = std::sqrt(b), nb = std::sqrt(c);
        if (na == 0.0 || nb == 0.0) return 0.0;
        return a / (na * nb);
    }
    double a = -0.0;
    if (metric == vl::EUCLIDEAN) {
        for (uint32_t i = 0; i < dim; ++i) {
            const double d = x[i] - y[i];
            a += d * d;
        }
        return 1.0 / (1.0 + std::sqrt(a));
    }
    for (uint32_t i = 0; i < dim; ++i) a += x[i] * y[i];
    return a;
}

struct Query {
    int n_cand = 0;
    float key[KP];
    uint32_t pos[KP];
    double score[KP];
    double q_norm = 1.0;
};

struct Expect {
    uint32_t n_out = 0, flags = 0;
    uint32_t pos[KP];
    double score[KP];
};

// The contract, restated: rank by (score desc, position asc); the certified prefix is every candidate scoring above B, or
// the whole list when it holds all n_rows <= 64 rows; settled iff no NaN and the prefix holds n_need candidates; then the
// greedy selection over the first n_need ranked candidates.
Expect model(const Query& q, int metric, uint64_t n_rows, uint32_t n_need, uint32_t k, double lambda, uint32_t dim, uint32_t ld,
             double R, double in_extra, const std::vector<double>& master)
{
    Expect e;
    bool nan = false;
    for (int i = 0; i < q.n_cand; ++i) nan = nan || q.score[i] != q.score[i];
    if (nan) e.flags |= vl::RESULT_HAS_NAN | vl::RESULT_NEEDS_EXACT;
    std::vector<int> order(q.n_cand);
    for (int i = 0; i < q.n_cand; ++i) order[i] = i;
    size_t certified = 0;
    if (!nan)
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            return q.score[a] > q.score[b] || (q.score[a] == q.score[b] && q.pos[a] < q.pos[b]);
        });
    if (n_rows <= (uint64_t)KP) {
        const bool complete = (uint64_t)q.n_cand >= n_rows;
        if (!complete) e.flags |= vl::RESULT_NEEDS_EXACT;
        if (complete && !nan) certified = order.size();
    } else if (q.n_cand < KP) {
        e.flags |= vl::RESULT_NEEDS_EXACT;
    } else if (!nan) {
        const double B = bound(metric, q.key[KP - 1], ld, R, q.q_norm, in_extra);
        while (certified < order.size() && q.score[order[certified]] > B) ++certified;
    }
    if (certified < n_need) e.flags |= vl::RESULT_NEEDS_EXACT;
    if (e.flags != 0) return e;  // handed back: nothing but the count (0) and the flags is written

    const uint32_t n = n_need;
    std::vector<double> rel(n);
    std::vector<const double*> row(n);
    for (uint32_t i = 0; i < n; ++i) {
        rel[i] = q.score[order[i]];
        row[i] = master.data() + (size_t)q.pos[order[i]] * dim;
    }
    const double one_minus = 1.0 - lambda;
    std::vector<uint32_t> sel{0};
    std::vector<char> chosen(n, 0);
    std::vector<double> red(n, -std::numeric_limits<double>::infinity());
    chosen[0] = 1;
    const uint32_t n_sel = k < n ? k : n;
    while (sel.size() < n_sel) {
        const uint32_t j = sel.back();
        for (uint32_t i = 0; i < n; ++i) {
            if (chosen[i]) continue;
            const double s = i < j ? calculate(metric, row[i], row[j], dim) : calculate(metric, row[j], row[i], dim);
            if (s > red[i]) red[i] = s;
        }
        int best = -1;
        double v_best = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            if (chosen[i]) continue;
            const double t1 = lambda * rel[i], t2 = one_minus * red[i];
            const double v = t1 - t2;
            if (best < 0 || v > v_best) {
                best = (int)i;
                v_best = v;
            }
        }
        sel.push_back((uint32_t)best);
        chosen[best] = 1;
    }
    e.n_out = n_sel;
    for (uint32_t t = 0; t < n_sel; ++t) {
        e.pos[t] = q.pos[order[sel[t]]];
        e.score[t] = rel[sel[t]];
    }
    return e;
}

uint64_t bits(double d)
{
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

std::map<std::string, long> g_seen;  // how often each kind of case was judged

// One launch: nq queries under one (metric, k, fetch_k, lambda, dim, n_rows).  Returns the number of mismatching queries.
int run_launch(std::mt19937_64& rng, int metric, uint32_t k, uint32_t fetch_k, double lambda, uint32_t dim, uint64_t n_rows, int nq)
{
    const uint32_t ld = (dim + 3u) & ~3u;
    const double R = 1.5, in_extra = vl::IN_EXTRA_MFMA;
    const uint32_t index_rows = (uint32_t)nq * SLOTS;
    const uint32_t n_need = (uint32_t)std::min<uint64_t>(fetch_k, n_rows);
    std::vector<double> master((size_t)index_rows * dim);
    for (double& v : master) v = (double)((int)(rng() % 4001) - 2000) / 1024.0;
    std::vector<Query> qs(nq);
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    for (int qi = 0; qi < nq; ++qi) {
        Query& q = qs[qi];
        // how many candidates: the complete list of a small S, one row short of it, or the list lengths
        if (n_rows <= (uint64_t)KP) q.n_cand = pick({(int)n_rows, (int)n_rows, (int)n_rows, (int)n_rows, (int)n_rows - 1, 0});
        else q.n_cand = pick({64, 64, 64, 64, 64, 64, 64, 63, 2, 1, 0});
        if (q.n_cand > (int)n_rows) q.n_cand = (int)n_rows;
        if (q.n_cand < 0) q.n_cand = 0;
        g_seen["n_cand " + std::string(q.n_cand == 0 ? "0" : q.n_cand == 1 ? "1" : q.n_cand == 2 ? "2" : q.n_cand == 63 ? "63" : q.n_cand == 64 ? "64" : "other")]++;
        // positions: distinct, in no order, inside the query's own slots
        std::vector<uint32_t> slots(SLOTS);
        for (int i = 0; i < SLOTS; ++i) slots[i] = (uint32_t)(qi * SLOTS + i);
        std::shuffle(slots.begin(), slots.end(), rng);
        for (int i = 0; i < KP; ++i) {
            q.pos[i] = i < q.n_cand ? slots[i] : vl::POS_SENTINEL;
            q.key[i] = i < q.n_cand ? 0.75f - 0.001f * (float)i : -std::numeric_limits<float>::infinity();
            q.score[i] = 0.0;
        }
        q.q_norm = metric == vl::COSINE && rng() % 16 == 0 ? 0.0 : 1.25;  // a zero query under cosine: B = +inf
        if (q.q_norm == 0.0) g_seen["zero cosine query"]++;
        // scores around B: all below, all above, exactly n_need or n_need - 1 above, a random cut; or one score ON B
        const double B = q.n_cand == KP ? bound(metric, q.key[KP - 1], ld, R, q.q_norm, in_extra) : 0.5;
        const double Bf = std::isfinite(B) ? B : 0.5;
        const int place = (int)(rng() % 8);
        int cut = 0;  // candidates [0, cut) lie above B
        const char* what = "";
        switch (place) {
        case 0: cut = 0; what = "B above every score"; break;
        case 1: cut = q.n_cand; what = "B below every score"; break;
        case 2: case 3: cut = (int)n_need; what = "B between ranks n - 1 and n"; break;
        case 4: cut = (int)n_need - 1; what = "B between ranks n - 2 and n - 1"; break;
        case 5: cut = (int)n_need; what = "the score of rank n on B"; break;
        case 6: cut = (int)n_need - 1; what = "the score of rank n - 1 on B"; break;
        default: cut = q.n_cand ? (int)(rng() % (q.n_cand + 1)) : 0; what = "B at a random rank"; break;
        }
        cut = std::max(0, std::min(cut, q.n_cand));
        g_seen[what]++;
        for (int i = 0; i < q.n_cand; ++i)
            q.score[i] = i < cut ? Bf + 1e-3 * (double)(1 + (rng() % 40)) : Bf - 1e-3 * (double)(1 + (rng() % 40));
        if ((place == 5 || place == 6) && cut < q.n_cand) q.score[cut] = Bf;  // exactly B: not certified
        bool out_of_order = false;  // (the draws above repeat values often)
        for (int i = 0; i < q.n_cand && !out_of_order; ++i)
            for (int j = 0; j < i && !out_of_order; ++j) out_of_order = q.score[i] == q.score[j] && (q.pos[i] < q.pos[j]) != (i < j);
        if (out_of_order) g_seen["equal scores, positions out of order"]++;
        if (q.n_cand && rng() % 12 == 0) {
            q.score[rng() % q.n_cand] = std::nan("");
            g_seen["one NaN score"]++;
        }
        // rows: independent, or copies of one row among the candidates (similarity ties resolve by rank)
        const int copies = (int)(rng() % 4);
        if (copies == 0 && q.n_cand >= 2) {
            g_seen["identical rows"]++;
            const double* src = master.data() + (size_t)q.pos[0] * dim;
            for (int i = 1; i < q.n_cand; ++i)
                if (rng() % 2) std::copy_n(src, dim, master.data() + (size_t)q.pos[i] * dim);
        }
        if (q.n_cand && rng() % 24 == 0) {  // a similarity that is not a number (or infinite) never replaces `red`
            master[(size_t)q.pos[rng() % q.n_cand] * dim + rng() % dim] = std::numeric_limits<double>::infinity();
            g_seen["a non-finite row value"]++;
        }
    }
    // device buffers
    std::vector<Cand32> h_lists((size_t)nq * KP);
    std::vector<double> h_scores((size_t)nq * KP), h_norms(nq);
    for (int qi = 0; qi < nq; ++qi) {
        for (int i = 0; i < KP; ++i) {
            h_lists[(size_t)qi * KP + i] = {qs[qi].key[i], qs[qi].pos[i]};
            h_scores[(size_t)qi * KP + i] = qs[qi].score[i];
        }
        h_norms[qi] = qs[qi].q_norm;
    }
    Cand32* d_lists;
    double *d_scores, *d_norms, *d_master;
    SearchResultBlock *d_ranked, *d_out;
    const size_t out_bytes = (size_t)(nq + 1) * sizeof(SearchResultBlock);  // one guard block
    HIP_OK(hipMalloc(&d_lists, h_lists.size() * sizeof(Cand32)));
    HIP_OK(hipMalloc(&d_scores, h_scores.size() * sizeof(double)));
    HIP_OK(hipMalloc(&d_norms, h_norms.size() * sizeof(double)));
    HIP_OK(hipMalloc(&d_master, master.size() * sizeof(double)));
    HIP_OK(hipMalloc(&d_ranked, out_bytes));
    HIP_OK(hipMalloc(&d_out, out_bytes));
    HIP_OK(hipMemcpy(d_lists, h_lists.data(), h_lists.size() * sizeof(Cand32), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_scores, h_scores.data(), h_scores.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_norms, h_norms.data(), h_norms.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_master, master.data(), master.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_ranked, 0xA5, out_bytes));
    HIP_OK(hipMemset(d_out, 0xA5, out_bytes));
    HIP_OK(vl::launch_mmr_batch(nullptr, metric, d_lists, d_scores, nq, d_norms, d_master, dim, n_rows, index_rows, n_need, k, lambda, R,
                                in_extra, d_ranked, d_out));
    HIP_OK(hipDeviceSynchronize());
    std::vector<SearchResultBlock> out(nq + 1), ranked(nq + 1);
    HIP_OK(hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ranked.data(), d_ranked, out_bytes, hipMemcpyDeviceToHost));
    for (void* p : {(void*)d_lists, (void*)d_scores, (void*)d_norms, (void*)d_master, (void*)d_ranked, (void*)d_out}) HIP_OK(hipFree(p));

    int bad = 0;
    uint64_t fill64;
    std::memset(&fill64, 0xA5, sizeof fill64);
    for (int qi = 0; qi < nq; ++qi) {
        const Expect e = model(qs[qi], metric, n_rows, n_need, k, lambda, dim, ld, R, in_extra, master);
        const SearchResultBlock& r = out[qi];
        bool ok = r.n_out == e.n_out && r.flags == e.flags && r.seq == FILL && r.pad == FILL;
        for (uint32_t i = 0; ok && i < (uint32_t)KP; ++i) {
            if (i < e.n_out) ok = r.pos[i] == e.pos[i] && bits(r.score[i]) == bits(e.score[i]);
            else ok = r.pos[i] == FILL && bits(r.score[i]) == fill64;  // untouched
        }
        if (e.flags == 0) g_seen["settled"]++;
        else g_seen["handed back"]++;
        if (!ok) {
            ++bad;
            std::printf("MISMATCH metric %d k %u fetch_k %u lambda %g dim %u n_rows %llu nq %d query %d: n_cand %d, device n_out %u flags %u, "
                        "model n_out %u flags %u\n",
                        metric, k, fetch_k, lambda, dim, (unsigned long long)n_rows, nq, qi, qs[qi].n_cand, r.n_out, r.flags, e.n_out,
                        e.flags);
            for (uint32_t i = 0; i < e.n_out && i < 12; ++i)
                std::printf("    [%u] device %u %016llx  model %u %016llx\n", i, r.pos[i], (unsigned long long)bits(r.score[i]), e.pos[i],
                            (unsigned long long)bits(e.score[i]));
        }
    }
    for (const SearchResultBlock* blocks : {out.data(), ranked.data()}) {
        const unsigned char* guard = reinterpret_cast<const unsigned char*>(&blocks[nq]);
        for (size_t i = 0; i < sizeof(SearchResultBlock); ++i)
            if (guard[i] != 0xA5) {
                std::printf("GUARD block behind query %d written (metric %d k %u)\n", nq - 1, metric, k);
                return bad + 1;
            }
    }
    return bad;
}

int audit()
{
    std::mt19937_64 rng(27);
    long launches = 0, queries = 0;
    int bad = 0;
    const uint32_t kf[6][2] = {{1, 1}, {2, 2}, {4, 20}, {20, 20}, {10, 60}, {60, 60}};
    const double lambdas[4] = {0.0, 0.25, 0.5, 1.0};
    const uint32_t dims[5] = {1, 3, 33, 384, 768};  // 33: one column behind a chunk; 1, 3: a single short chunk
    for (int metric : {vl::COSINE, vl::EUCLIDEAN, vl::DOT}) {
        long c = 0;
        for (const auto& p : kf)
            for (uint64_t n_rows : {1ull, 40ull, 64ull, 65ull, 100000ull})
                for (int nq : {1, 5, 131}) {  // 131: the last workgroup of four ranking waves is partly empty
                    const uint32_t dim = dims[c % 5];
                    const double lambda = lambdas[(c / 5) % 4];
                    ++c;
                    g_seen["metric " + std::to_string(metric) + " dim " + std::to_string(dim)]++;
                    g_seen["metric " + std::to_string(metric) + " lambda " + std::to_string(lambda)]++;
                    bad += run_launch(rng, metric, p[0], p[1], lambda, dim, n_rows, nq);
                    ++launches;
                    queries += nq;
                }
    }
    for (const auto& kv : g_seen) std::printf("  %-44s %ld\n", kv.first.c_str(), kv.second);
    std::vector<std::string> must = {"n_cand 0", "n_cand 1", "n_cand 2", "n_cand 63", "n_cand 64", "B above every score",
                                     "B below every score", "B between ranks n - 1 and n", "B between ranks n - 2 and n - 1",
                                     "the score of rank n on B", "the score of rank n - 1 on B", "equal scores, positions out of order",
                                     "identical rows", "one NaN score", "zero cosine query", "settled", "handed back"};
    for (int metric : {vl::COSINE, vl::EUCLIDEAN, vl::DOT}) {
        for (uint32_t d : dims) must.push_back("metric " + std::to_string(metric) + " dim " + std::to_string(d));
        for (double l : lambdas) must.push_back("metric " + std::to_string(metric) + " lambda " + std::to_string(l));
    }
    for (const std::string& m : must)
        if (g_seen[m] == 0) {
            std::printf("case kind never judged: %s\n", m.c_str());
            ++bad;
        }
    std::printf("mmr batch: %ld queries in %ld launches, %d mismatches\n", queries, launches, bad);
    return bad;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "stage") {
        if (audit()) return 1;
        std::printf("audit ok\n");
        return 0;
    }
    std::printf("usage: mmr_batch_audit stage\n");
    return 2;
}
