// Audit of the batched grouped search's two kernels on inputs handed to them directly.  From outside
// (tests/test_gpu_grouped_batch.py) a query the collapse stage flags without need, or settles with the right rows for the
// wrong reason, stays green: the single call re-answers it, or the data never reach the edge.  Here
//   grouped_batch_audit collapse
//       feeds k_batch_rank_collapse (through launch_batch_rank_collapse of the library) hand-made candidate lists, scores and
//       group_of_row tables and compares EVERY word of every result block -- entries, count, flags, the words it must not
//       touch and a guard block behind the last query -- with the host model below, which evaluates bound_for_key from
//       score_bound.hpp, the function the device uses;
//   grouped_batch_audit keepbits <cases> <out>
//       runs k_group_keep_bits on the cases of a file and dumps bitmap (with guard words) and count for the caller to judge.
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

#include "../../vectorlite_amd/csrc/group_plan.hpp"
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
using vl::GroupedResultBlock;
using vl::KP;

constexpr uint32_t FILL = 0xA5A5A5A5u;
constexpr int SLOTS = 128;  // storage positions reserved per query: its 64 candidates are drawn from them

double bound(int metric, float key, uint32_t ld, double R, double Q, double in_extra)
{
    switch (metric) {
    case vl::COSINE: return vl::bound_for_key<vl::BOUND_COSINE>(key, ld, R, Q, in_extra);
    case vl::EUCLIDEAN: return vl::bound_for_key<vl::BOUND_EUCLIDEAN>(key, ld, R, Q, in_extra);
    default: return vl::bound_for_key<vl::BOUND_DOT>(key, ld, R, Q, in_extra);
    }
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
    uint32_t pos[KP], group[KP];
    double score[KP];
};

// The contract, restated: rank by (score desc, position asc); the certified prefix is every candidate scoring above B, or
// the whole list when it holds all n_rows <= 64 rows; walk the prefix, keep the first row of each group, emit the first k.
Expect model(const Query& q, int metric, uint64_t n_rows, uint32_t k, uint32_t ld, double R, double in_extra,
             const std::vector<uint32_t>& gor)
{
    Expect e;
    bool nan = false;
    for (int i = 0; i < q.n_cand; ++i) nan = nan || q.score[i] != q.score[i];
    if (nan) e.flags |= vl::RESULT_HAS_NAN | vl::RESULT_NEEDS_EXACT;
    std::vector<int> order(q.n_cand);
    for (int i = 0; i < q.n_cand; ++i) order[i] = i;
    size_t certified = 0;
    bool complete = false;
    if (!nan)
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            return q.score[a] > q.score[b] || (q.score[a] == q.score[b] && q.pos[a] < q.pos[b]);
        });
    if (n_rows <= (uint64_t)KP) {
        complete = (uint64_t)q.n_cand >= n_rows;
        if (!complete) e.flags |= vl::RESULT_NEEDS_EXACT;
        if (complete && !nan) certified = order.size();
    } else if (q.n_cand < KP) {
        e.flags |= vl::RESULT_NEEDS_EXACT;
    } else if (!nan) {
        const double B = bound(metric, q.key[KP - 1], ld, R, q.q_norm, in_extra);
        while (certified < order.size() && q.score[order[certified]] > B) ++certified;
    }
    for (size_t i = 0; i < certified; ++i)
        if (gor[q.pos[order[i]]] == vl::GROUP_NONE) {  // a certified row without a group: nothing is emitted, hand back
            e.flags |= vl::RESULT_NEEDS_EXACT;
            certified = 0;
        }
    std::vector<uint32_t> seen;
    uint32_t n_first = 0;
    for (size_t i = 0; i < certified; ++i) {
        const uint32_t g = gor[q.pos[order[i]]];
        if (std::find(seen.begin(), seen.end(), g) != seen.end()) continue;
        seen.push_back(g);
        if (n_first < k) {
            e.pos[n_first] = q.pos[order[i]];
            e.group[n_first] = g;
            e.score[n_first] = q.score[order[i]];
        }
        ++n_first;
    }
    e.n_out = n_first < k ? n_first : k;
    if (n_first < k && !(complete && !nan)) e.flags |= vl::RESULT_NEEDS_EXACT;
    return e;
}

uint64_t bits(double d)
{
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

std::map<std::string, long> g_seen;  // how often each kind of case was judged

// One launch: nq queries under one (metric, k, n_rows).  Returns the number of mismatching queries.
int run_launch(std::mt19937_64& rng, int metric, uint32_t k, uint64_t n_rows, int nq)
{
    const uint32_t ld = 128;
    const double R = 1.5, in_extra = vl::IN_EXTRA_MFMA;
    const uint32_t index_rows = (uint32_t)nq * SLOTS;
    std::vector<uint32_t> gor(index_rows, vl::GROUP_NONE);
    std::vector<Query> qs(nq);
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    for (int qi = 0; qi < nq; ++qi) {
        Query& q = qs[qi];
        // how many candidates: the complete list of a small S, one row short of it, or the four list lengths
        if (n_rows <= (uint64_t)KP) q.n_cand = pick({(int)n_rows, (int)n_rows, (int)n_rows, (int)n_rows - 1, 0});
        else q.n_cand = pick({64, 64, 64, 64, 64, 63, 1, 0});
        if (q.n_cand > (int)n_rows) q.n_cand = (int)n_rows;
        g_seen["n_cand " + std::to_string(q.n_cand == 0 ? 0 : q.n_cand == 1 ? 1 : q.n_cand == 63 ? 63 : q.n_cand == 64 ? 64 : 2)]++;
        // positions: distinct, in no order, inside the query's own slots
        std::vector<uint32_t> slots(SLOTS);
        for (int i = 0; i < SLOTS; ++i) slots[i] = (uint32_t)(qi * SLOTS + i);
        std::shuffle(slots.begin(), slots.end(), rng);
        for (int i = 0; i < KP; ++i) {
            q.pos[i] = i < q.n_cand ? slots[i] : vl::POS_SENTINEL;
            q.key[i] = i < q.n_cand ? 0.75f - 0.001f * (float)i : -std::numeric_limits<float>::infinity();
            q.score[i] = 0.0;
        }
        // groups: all in one, each its own, or runs of 2-5
        const int grouping = (int)(rng() % 3);
        g_seen[grouping == 0 ? "one group" : grouping == 1 ? "own groups" : "groups of 2-5"]++;
        uint32_t g = (uint32_t)qi * KP, left = 0;
        for (int i = 0; i < q.n_cand; ++i) {
            if (grouping == 1 || (grouping == 2 && left == 0)) {
                ++g;
                left = 2 + (uint32_t)(rng() % 4);
            }
            if (left) --left;
            gor[q.pos[i]] = g;
        }
        q.q_norm = metric == vl::COSINE && rng() % 16 == 0 ? 0.0 : 1.25;  // a zero query under cosine: B = +inf
        if (q.q_norm == 0.0) g_seen["zero cosine query"]++;
        // scores around B: all below, all above, a cut between two ranks, one exactly ON B (not certified)
        const double B = q.n_cand == KP ? bound(metric, q.key[KP - 1], ld, R, q.q_norm, in_extra) : 0.5;
        const double Bf = std::isfinite(B) ? B : 0.5;
        const int place = (int)(rng() % 4);
        const int cut = q.n_cand ? (int)(rng() % q.n_cand) : 0;  // candidates [0, cut) lie above B
        g_seen[place == 0 ? "B above every score" : place == 1 ? "B below every score" : place == 2 ? "B between ranks" : "a score equal to B"]++;
        for (int i = 0; i < q.n_cand; ++i) {
            const bool above = place == 1 || (place >= 2 && i < cut);
            q.score[i] = above ? Bf + 1e-3 * (double)(1 + (rng() % 40)) : Bf - 1e-3 * (double)(1 + (rng() % 40));
        }
        if (place == 3 && q.n_cand) {
            q.score[cut] = Bf;  // exactly B
            if (cut + 1 < q.n_cand) q.score[cut + 1] = std::nextafter(Bf, 2.0 * std::fabs(Bf) + 1.0);  // and the next double above it
        }
        // (the draws above repeat values often: equal scores whose positions are out of order)
        for (int i = 0; i < q.n_cand; ++i)
            for (int j = 0; j < i; ++j)
                if (q.score[i] == q.score[j] && (q.pos[i] < q.pos[j]) != (i < j)) {
                    g_seen["equal scores, positions out of order"]++;
                    i = j = q.n_cand;
                }
        if (q.n_cand && rng() % 12 == 0) {
            q.score[rng() % q.n_cand] = std::nan("");
            g_seen["one NaN"]++;
        }
        if (q.n_cand == KP && rng() % 40 == 0) {  // a candidate the table gives no group
            gor[q.pos[rng() % KP]] = vl::GROUP_NONE;
            g_seen["a row without a group"]++;
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
    double *d_scores, *d_norms;
    uint32_t* d_gor;
    GroupedResultBlock* d_out;
    const size_t out_bytes = (size_t)(nq + 1) * sizeof(GroupedResultBlock);  // one guard block
    HIP_OK(hipMalloc(&d_lists, h_lists.size() * sizeof(Cand32)));
    HIP_OK(hipMalloc(&d_scores, h_scores.size() * sizeof(double)));
    HIP_OK(hipMalloc(&d_norms, h_norms.size() * sizeof(double)));
    HIP_OK(hipMalloc(&d_gor, gor.size() * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&d_out, out_bytes));
    HIP_OK(hipMemcpy(d_lists, h_lists.data(), h_lists.size() * sizeof(Cand32), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_scores, h_scores.data(), h_scores.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_norms, h_norms.data(), h_norms.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_gor, gor.data(), gor.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xA5, out_bytes));
    HIP_OK(vl::launch_batch_rank_collapse(nullptr, metric, d_lists, d_scores, nq, d_norms, ld, n_rows, k, R, d_gor, index_rows, d_out,
                                          in_extra));
    HIP_OK(hipDeviceSynchronize());
    std::vector<GroupedResultBlock> out(nq + 1);
    HIP_OK(hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
    for (void* p : {(void*)d_lists, (void*)d_scores, (void*)d_norms, (void*)d_gor, (void*)d_out}) HIP_OK(hipFree(p));

    int bad = 0;
    uint64_t fill64;
    std::memset(&fill64, 0xA5, sizeof fill64);
    for (int qi = 0; qi < nq; ++qi) {
        const Expect e = model(qs[qi], metric, n_rows, k, ld, R, in_extra, gor);
        const GroupedResultBlock& r = out[qi];
        bool ok = r.n_out == e.n_out && r.flags == e.flags;
        for (uint32_t i = 0; ok && i < (uint32_t)KP; ++i) {
            if (i < e.n_out) ok = r.pos[i] == e.pos[i] && r.group[i] == e.group[i] && bits(r.score[i]) == bits(e.score[i]);
            else ok = r.pos[i] == FILL && r.group[i] == FILL && bits(r.score[i]) == fill64;  // untouched
        }
        if (e.flags == 0) g_seen[e.n_out == k ? "settled with k groups" : "settled complete with fewer than k groups"]++;
        else g_seen["handed back"]++;
        if (!ok) {
            ++bad;
            std::printf("MISMATCH metric %d k %u n_rows %llu nq %d query %d: n_cand %d, device n_out %u flags %u, model n_out %u flags %u\n",
                        metric, k, (unsigned long long)n_rows, nq, qi, qs[qi].n_cand, r.n_out, r.flags, e.n_out, e.flags);
        }
    }
    const unsigned char* guard = reinterpret_cast<const unsigned char*>(&out[nq]);
    for (size_t i = 0; i < sizeof(GroupedResultBlock); ++i)
        if (guard[i] != 0xA5) {
            std::printf("GUARD block behind query %d written (metric %d k %u)\n", nq - 1, metric, k);
            return bad + 1;
        }
    return bad;
}

int collapse_audit()
{
    std::mt19937_64 rng(26);
    long launches = 0, queries = 0;
    int bad = 0;
    for (int metric : {vl::COSINE, vl::EUCLIDEAN, vl::DOT})
        for (uint32_t k : {1u, 10u, 60u})
            for (uint64_t n_rows : {1ull, 40ull, 64ull, 65ull, 100000ull})
                for (int nq : {1, 5, 131}) {  // 131: the last workgroup of four waves is partly empty
                    bad += run_launch(rng, metric, k, n_rows, nq);
                    ++launches;
                    queries += nq;
                }
    for (const auto& kv : g_seen) std::printf("  %-44s %ld\n", kv.first.c_str(), kv.second);
    const char* must[] = {"n_cand 0", "n_cand 1", "n_cand 63", "n_cand 64", "one group", "own groups", "groups of 2-5",
                          "B above every score", "B below every score", "B between ranks", "a score equal to B",
                          "equal scores, positions out of order", "one NaN", "zero cosine query", "a row without a group",
                          "settled with k groups", "settled complete with fewer than k groups", "handed back"};
    for (const char* m : must)
        if (g_seen[m] == 0) {
            std::printf("case kind never judged: %s\n", m);
            ++bad;
        }
    std::printf("collapse: %ld queries in %ld launches, %d mismatches\n", queries, launches, bad);
    return bad;
}

// ---- k_group_keep_bits: cases from a file, raw outputs to a file ----------------------------------------------------------
// case: u64 n, u64 mode (0 table only, 1 an exclusion bitmap, 2 an include id set), u64 nf; u32 group_of_row[n] (padded to 8
// bytes); mode 1: u64 filter_keep[(n + 63) / 64]; mode 2: u64 pos_ids[n], u64 fids[nf].
// output per case: u64 m, u64 words, then words + 2 u64: the bitmap and two guard words behind it.
int keepbits(const char* in_path, const char* out_path)
{
    FILE* fi = std::fopen(in_path, "rb");
    FILE* fo = std::fopen(out_path, "wb");
    if (!fi || !fo) return 3;
    uint64_t n_cases = 0;
    if (std::fread(&n_cases, 8, 1, fi) != 1) return 3;
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t hdr[3];
        if (std::fread(hdr, 8, 3, fi) != 3) return 3;
        const uint64_t n = hdr[0], mode = hdr[1], nf = hdr[2], words = (n + 63) / 64;
        std::vector<uint32_t> gor((n + 1) & ~1ull);
        if (std::fread(gor.data(), 4, gor.size(), fi) != gor.size()) return 3;
        std::vector<uint64_t> fkeep(mode == 1 ? words : 0), pos_ids(mode == 2 ? n : 0), fids(mode == 2 ? nf : 0);
        if (!fkeep.empty() && std::fread(fkeep.data(), 8, fkeep.size(), fi) != fkeep.size()) return 3;
        if (!pos_ids.empty() && std::fread(pos_ids.data(), 8, pos_ids.size(), fi) != pos_ids.size()) return 3;
        if (!fids.empty() && std::fread(fids.data(), 8, fids.size(), fi) != fids.size()) return 3;
        uint32_t *d_gor, *d_m;
        unsigned long long *d_fkeep = nullptr, *d_pos = nullptr, *d_fids = nullptr, *d_keep;
        HIP_OK(hipMalloc(&d_gor, gor.size() * 4));
        HIP_OK(hipMemcpy(d_gor, gor.data(), gor.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMalloc(&d_m, 4));
        HIP_OK(hipMemset(d_m, 0xA5, 4));  // the launcher zeroes it
        HIP_OK(hipMalloc(&d_keep, (words + 2) * 8));
        HIP_OK(hipMemset(d_keep, 0xA5, (words + 2) * 8));
        if (mode == 1) {
            HIP_OK(hipMalloc(&d_fkeep, words * 8));
            HIP_OK(hipMemcpy(d_fkeep, fkeep.data(), words * 8, hipMemcpyHostToDevice));
        }
        if (mode == 2) {
            HIP_OK(hipMalloc(&d_pos, n * 8));
            HIP_OK(hipMemcpy(d_pos, pos_ids.data(), n * 8, hipMemcpyHostToDevice));
            HIP_OK(hipMalloc(&d_fids, (nf ? nf : 1) * 8));
            if (nf) HIP_OK(hipMemcpy(d_fids, fids.data(), nf * 8, hipMemcpyHostToDevice));
        }
        HIP_OK(vl::launch_group_keep_bits(nullptr, d_gor, n, d_fkeep, d_pos, d_fids, nf, d_keep, d_m));
        HIP_OK(hipDeviceSynchronize());
        uint32_t m32 = 0;
        std::vector<uint64_t> out(words + 2);
        HIP_OK(hipMemcpy(&m32, d_m, 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(out.data(), d_keep, (words + 2) * 8, hipMemcpyDeviceToHost));
        const uint64_t head[2] = {m32, words};
        std::fwrite(head, 8, 2, fo);
        std::fwrite(out.data(), 8, out.size(), fo);
        for (void* p : {(void*)d_gor, (void*)d_m, (void*)d_keep, (void*)d_fkeep, (void*)d_pos, (void*)d_fids})
            if (p) HIP_OK(hipFree(p));
    }
    std::fclose(fi);
    std::fclose(fo);
    std::printf("keepbits: %llu cases run\n", (unsigned long long)n_cases);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "collapse") {
        if (collapse_audit()) return 1;
        std::printf("audit ok\n");
        return 0;
    }
    if (argc == 4 && std::string(argv[1]) == "keepbits") {
        if (keepbits(argv[2], argv[3])) return 1;
        std::printf("audit ok\n");
        return 0;
    }
    std::printf("usage: grouped_batch_audit collapse | keepbits <cases> <out>\n");
    return 2;
}
