// hnsw_graph_check.hpp -- invariants of the HNSW graph the batched GPU build leaves behind (HNSW section).
// Plain C++17 on host copies of the graph arrays: no HIP, no product header.  Used by hnsw_graph_check_test.cpp (CPU,
// hand-made graphs, under ASan + UBSan) and by hnsw_graph_audit.hip (the arrays of a real index after every mutation).
//
// Two pieces of the product are RESTATED here, not included:
//   level_law()      hnsw_index.cpp: draw_level  (splitmix64 of seed * 0x100000001B3 + node, floor(-ln u / ln m), 0..15)
//   edge_key_f32()   hnsw.hip: row_distance_f32 + walk_key, the f32 distance the build stores with every edge
// Compile with -ffp-contract=off: every product and sum below rounds on its own unless fmaf() spells the fusion out.
//
// check() returns the first violation as text ("G4: ... node 7 layer 0 slot 3 ...") or an empty string.
//   G1  level[] (device and host) follows the level law; upper_off[] is the exclusive prefix sum of the levels, n_upper
//       their total; g_cap >= n, u_cap >= n_upper
//   G2  max_level = max(level), entry = the first node of that level
//   G3  cnt0 <= m0, cntU <= m; a listed neighbour is < n, is not the owner, and has level >= the list's layer (the walk
//       would read another node's upper slot otherwise).  A node owns exactly level[i] upper slots (G1), so it can list
//       nothing above its own level
//   G4  no list names a node twice
//   G5  every stored edge distance is, as bits, edge_key_f32(larger index as the query row, smaller as the candidate)
//   G6  indeg0[v] = number of layer-0 entries naming v, and >= 1 for every node when n >= 2 (a caller may ask for the
//       nodes without an incoming edge to be counted instead: short lists cannot promise one to everybody)
//   G7  lock[] is zero over the whole capacity; cnt0 / indeg0 are zero in [n, g_cap), cntU in [n_upper, u_cap)
//   G8  device node_id / live equal the host's; id_to_node holds exactly the live ids; live_count agrees
//   G9  reported, not judged: nodes not reachable on layer 0 from the entry point, and whether layer 0 is strongly
//       connected (then every landing point of a descent reaches everything)
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace hgc {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int MAX_LEVEL = 15;
enum Metric : int { COSINE = 0, EUCLIDEAN = 1, MANHATTAN = 2, DOT = 3 };

inline uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// u = (top 53 bits + 1) / 2^53 in (0, 1]; level = floor(-ln(u) / ln(m)) clamped to 0 .. 15
inline int level_law(uint64_t seed, uint64_t node, uint32_t m)
{
    const uint64_t r = splitmix64(seed * 0x100000001B3ull + node);
    const double u = ((double)(r >> 11) + 1.0) * (1.0 / 9007199254740992.0);
    int l = (int)std::floor(-std::log(u) / std::log((double)m));
    if (l < 0) l = 0;
    if (l > MAX_LEVEL) l = MAX_LEVEL;
    return l;
}

// The f64 bit pattern of the scaled distance; negative, zero and NaN become 0.
inline uint64_t walk_key(double scaled)
{
    if (!(scaled > 0.0)) return 0ull;
    uint64_t u;
    std::memcpy(&u, &scaled, sizeof u);
    return u;
}

// Two lanes share a row: lane `half` takes the 16-byte chunks half, half + 2, ... in order, one sequential chain each;
// the halves are added; then the metric's tail.  q is the query row (the LARGER node index of an edge), r the candidate.
inline uint64_t edge_key_f32(int metric, const float* q, float q_inv, const float* r, float r_inv, uint32_t ld)
{
    float part[2];
    for (uint32_t half = 0; half < 2; ++half) {
        float s = 0.f;
        for (uint32_t c = half; c < ld / 4; c += 2) {
            const float* x = r + 4 * (size_t)c;
            const float* y = q + 4 * (size_t)c;
            if (metric == COSINE || metric == DOT) {
                s = fmaf(x[0], y[0], s); s = fmaf(x[1], y[1], s); s = fmaf(x[2], y[2], s); s = fmaf(x[3], y[3], s);
            } else if (metric == EUCLIDEAN) {
                const float a = x[0] - y[0], b = x[1] - y[1], cc = x[2] - y[2], d = x[3] - y[3];
                s = fmaf(a, a, s); s = fmaf(b, b, s); s = fmaf(cc, cc, s); s = fmaf(d, d, s);
            } else {
                const float t = fabsf(x[0] - y[0]) + fabsf(x[1] - y[1]) + fabsf(x[2] - y[2]) + fabsf(x[3] - y[3]);
                s = s + t;
            }
        }
        part[half] = s;
    }
    const float s = part[0] + part[1];
    double scaled;
    if (metric == COSINE) {
        if (r_inv == 0.f || q_inv == 0.f) {
            scaled = 1000.0;
        } else {
            const float cs = s * r_inv * q_inv;
            scaled = (1.0 - (double)cs) * 1000.0;
        }
    } else if (metric == EUCLIDEAN) {
        scaled = (double)sqrtf(s) * 1000.0;
    } else if (metric == MANHATTAN) {
        scaled = (double)s * 1000.0;
    } else {
        float d = s;
        d = d < -1000.f ? -1000.f : (d > 1000.f ? 1000.f : d);
        scaled = 1000.0 - (double)d;
    }
    return walk_key(scaled);
}

// Host copies of everything the invariants speak about.  Device arrays are copied over their whole capacity where the
// tail matters (G7); nbr / dist rows only over the nodes and slots in use (their tails are never read before written).
struct Graph {
    uint64_t n = 0;  // nodes, tombstoned ones included
    uint32_t m = 16, m0 = 32;
    int metric = EUCLIDEAN;
    uint32_t ld = 0;  // slab row stride in floats (a multiple of 4)
    uint64_t seed = 0;
    uint64_t g_cap = 0, u_cap = 0, n_upper = 0;
    uint32_t entry = NONE;
    int max_level = -1;
    // device
    std::vector<uint8_t> level;       // [g_cap]
    std::vector<uint32_t> upper_off;  // [g_cap]
    std::vector<uint32_t> cnt0;       // [g_cap]
    std::vector<uint32_t> lock;       // [g_cap]
    std::vector<uint32_t> indeg0;     // [g_cap]
    std::vector<uint32_t> nbr0;       // [n, m0]
    std::vector<uint64_t> dist0;      // [n, m0]
    std::vector<uint32_t> cntU;       // [u_cap]
    std::vector<uint32_t> nbrU;       // [n_upper, m]
    std::vector<uint64_t> distU;      // [n_upper, m]
    std::vector<uint64_t> node_id;    // [n]
    std::vector<uint8_t> live;        // [n]
    std::vector<float> slab;          // [n, ld]
    std::vector<float> inv_norm;      // [n]
    // host bookkeeping
    std::vector<uint8_t> h_level;
    std::vector<uint32_t> h_upper_off;
    std::vector<uint64_t> h_node_id;
    std::vector<uint8_t> h_live;
    std::vector<std::pair<uint64_t, uint32_t>> id_to_node;  // any order
    uint64_t live_count = 0;
};

struct Reach {
    uint64_t unreachable = 0;        // nodes a layer-0 flood from the entry point does not reach
    bool strongly_connected = true;  // every node also reaches the entry point
    uint64_t orphans = 0;            // nodes without an incoming layer-0 edge (only counted when check() is told to report them)
    std::vector<uint32_t> lost;      // the first unreachable nodes (at most 8)
};

namespace detail {
inline std::string at(const char* inv, const std::string& what, uint64_t node, int layer, int64_t slot)
{
    std::string s = std::string(inv) + ": " + what + " (node " + std::to_string(node) + ", layer " + std::to_string(layer);
    if (slot >= 0) s += ", slot " + std::to_string(slot);
    return s + ")";
}
inline uint64_t flood(uint64_t n, uint32_t start, const std::vector<std::vector<uint32_t>>& adj, std::vector<uint8_t>& seen)
{
    seen.assign(n, 0);
    std::vector<uint32_t> stack{start};
    seen[start] = 1;
    uint64_t got = 1;
    while (!stack.empty()) {
        const uint32_t v = stack.back();
        stack.pop_back();
        for (uint32_t e : adj[v])
            if (!seen[e]) {
                seen[e] = 1;
                ++got;
                stack.push_back(e);
            }
    }
    return got;
}
}  // namespace detail

// report_orphans: nodes without an incoming layer-0 edge are counted into reach->orphans instead of being a G6 violation
inline std::string check(const Graph& g, Reach* reach = nullptr, bool report_orphans = false)
{
    uint64_t orphans = 0;
    using detail::at;
    const uint64_t n = g.n;
    auto sized = [](size_t have, uint64_t need) { return (uint64_t)have >= need; };
    if (!sized(g.level.size(), g.g_cap) || !sized(g.upper_off.size(), g.g_cap) || !sized(g.cnt0.size(), g.g_cap) ||
        !sized(g.lock.size(), g.g_cap) || !sized(g.indeg0.size(), g.g_cap) || !sized(g.cntU.size(), g.u_cap))
        return "G1: a per-node array is shorter than the capacity it was copied for";

    // ---- G1
    if (g.g_cap < n) return "G1: g_cap " + std::to_string(g.g_cap) + " < n " + std::to_string(n);
    if (g.h_level.size() != n || g.h_upper_off.size() != n) return "G1: host level / upper_off do not hold n entries";
    uint64_t run = 0;
    int top = -1;
    uint32_t first_top = NONE;
    for (uint64_t i = 0; i < n; ++i) {
        const int want = level_law(g.seed, i, g.m);
        if (g.level[i] != want) return at("G1", "device level " + std::to_string(g.level[i]) + " != level law " + std::to_string(want), i, 0, -1);
        if (g.h_level[i] != want) return at("G1", "host level " + std::to_string(g.h_level[i]) + " != level law " + std::to_string(want), i, 0, -1);
        if (g.upper_off[i] != run) return at("G1", "device upper_off " + std::to_string(g.upper_off[i]) + " != prefix sum " + std::to_string(run), i, 0, -1);
        if (g.h_upper_off[i] != run) return at("G1", "host upper_off " + std::to_string(g.h_upper_off[i]) + " != prefix sum " + std::to_string(run), i, 0, -1);
        run += (uint64_t)want;
        if (want > top) {
            top = want;
            first_top = (uint32_t)i;
        }
    }
    if (g.n_upper != run) return "G1: n_upper " + std::to_string(g.n_upper) + " != total of the levels " + std::to_string(run);
    if (g.u_cap < g.n_upper) return "G1: u_cap " + std::to_string(g.u_cap) + " < n_upper " + std::to_string(g.n_upper);
    if (!sized(g.nbr0.size(), n * g.m0) || !sized(g.dist0.size(), n * g.m0) || !sized(g.nbrU.size(), run * g.m) ||
        !sized(g.distU.size(), run * g.m) || !sized(g.slab.size(), n * g.ld) || !sized(g.inv_norm.size(), n))
        return "G1: a list or row array is shorter than the nodes and slots in use";

    // ---- G2
    if (g.max_level != top) return "G2: max_level " + std::to_string(g.max_level) + " != max(level) " + std::to_string(top);
    if (g.entry != first_top) return "G2: entry " + std::to_string(g.entry) + " != first node of the top level " + std::to_string(first_top);

    // one pass over every list for G3, G4, G5; layer-0 in-degrees for G6
    std::vector<uint32_t> indeg(n, 0);
    std::vector<uint32_t> stamp(n, NONE);  // stamp[v] = serial of the last list that named v
    uint32_t serial = 0;
    for (int pass = 3; pass <= 5; ++pass) {  // a G3 violation anywhere is named before a G4 one, and so on
        for (uint64_t i = 0; i < n; ++i) {
            for (int layer = 0; layer <= (int)g.level[i]; ++layer) {
                const uint32_t cap = layer == 0 ? g.m0 : g.m;
                const uint64_t slot = layer == 0 ? i : (uint64_t)g.upper_off[i] + (uint64_t)(layer - 1);
                const uint32_t cnt = layer == 0 ? g.cnt0[i] : g.cntU[slot];
                const uint32_t* nb = layer == 0 ? &g.nbr0[i * g.m0] : &g.nbrU[slot * g.m];
                const uint64_t* nd = layer == 0 ? &g.dist0[i * g.m0] : &g.distU[slot * g.m];
                if (pass == 3 && cnt > cap) return at("G3", "count " + std::to_string(cnt) + " > capacity " + std::to_string(cap), i, layer, -1);
                ++serial;
                for (uint32_t t = 0; t < cnt && t < cap; ++t) {
                    const uint32_t v = nb[t];
                    if (pass == 3) {
                        if (v >= n) return at("G3", "neighbour " + std::to_string(v) + " >= n", i, layer, t);
                        if (v == i) return at("G3", "a node lists itself", i, layer, t);
                        if ((int)g.level[v] < layer) return at("G3", "neighbour " + std::to_string(v) + " of level " + std::to_string(g.level[v]) + " listed above its level", i, layer, t);
                    } else if (pass == 4) {
                        if (stamp[v] == serial) return at("G4", "neighbour " + std::to_string(v) + " named twice", i, layer, t);
                        stamp[v] = serial;
                        if (layer == 0) ++indeg[v];
                    } else {
                        const uint64_t a = i > v ? i : v, b = i > v ? v : i;
                        const uint64_t want = edge_key_f32(g.metric, &g.slab[a * g.ld], g.inv_norm[a], &g.slab[b * g.ld], g.inv_norm[b], g.ld);
                        if (nd[t] != want) {
                            char buf[96];
                            snprintf(buf, sizeof buf, "stored distance %016llx != f32 key %016llx of edge to %u", (unsigned long long)nd[t], (unsigned long long)want, v);
                            return at("G5", buf, i, layer, t);
                        }
                    }
                }
            }
        }
    }

    // ---- G6
    for (uint64_t v = 0; v < n; ++v) {
        if (g.indeg0[v] != indeg[v]) return at("G6", "indeg0 " + std::to_string(g.indeg0[v]) + " != " + std::to_string(indeg[v]) + " layer-0 entries naming the node", v, 0, -1);
        if (n >= 2 && indeg[v] == 0) {
            if (!report_orphans) return at("G6", "no incoming layer-0 edge", v, 0, -1);
            ++orphans;
        }
    }

    // ---- G7
    for (uint64_t i = 0; i < g.g_cap; ++i)
        if (g.lock[i] != 0) return at("G7", "lock held at rest", i, 0, -1);
    for (uint64_t i = n; i < g.g_cap; ++i) {
        if (g.cnt0[i] != 0) return at("G7", "cnt0 not zero beyond n", i, 0, -1);
        if (g.indeg0[i] != 0) return at("G7", "indeg0 not zero beyond n", i, 0, -1);
    }
    for (uint64_t s = g.n_upper; s < g.u_cap; ++s)
        if (g.cntU[s] != 0) return "G7: cntU not zero beyond n_upper (slot " + std::to_string(s) + ")";

    // ---- G8
    if (g.h_node_id.size() != n || g.h_live.size() != n || !sized(g.node_id.size(), n) || !sized(g.live.size(), n))
        return "G8: node_id / live do not hold n entries";
    uint64_t alive = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (g.node_id[i] != g.h_node_id[i]) return at("G8", "device node_id differs from the host's", i, 0, -1);
        if (g.live[i] != g.h_live[i] || g.live[i] > 1) return at("G8", "device live flag differs from the host's", i, 0, -1);
        alive += g.h_live[i];
    }
    if (g.live_count != alive) return "G8: live_count " + std::to_string(g.live_count) + " != live flags set " + std::to_string(alive);
    if (g.id_to_node.size() != alive) return "G8: id_to_node holds " + std::to_string(g.id_to_node.size()) + " ids, live nodes " + std::to_string(alive);
    {
        std::vector<uint8_t> named(n, 0);
        for (const auto& kv : g.id_to_node) {
            const uint32_t v = kv.second;
            if (v >= n || !g.h_live[v] || g.h_node_id[v] != kv.first || named[v])
                return "G8: id_to_node maps id " + std::to_string(kv.first) + " to node " + std::to_string(v) + ", which is not the live node of that id";
            named[v] = 1;
        }
    }

    // ---- G9 (reported)
    if (reach) {
        *reach = Reach{};
        reach->orphans = orphans;
        if (n >= 1) {
            std::vector<uint8_t> seen;
            std::vector<std::vector<uint32_t>> fwd(n), rev(n);
            for (uint64_t i = 0; i < n; ++i)
                for (uint32_t t = 0; t < g.cnt0[i]; ++t) {
                    const uint32_t v = g.nbr0[i * g.m0 + t];
                    fwd[i].push_back(v);
                    rev[v].push_back((uint32_t)i);
                }
            reach->unreachable = n - detail::flood(n, g.entry, fwd, seen);
            for (uint64_t i = 0; i < n && reach->lost.size() < 8; ++i)
                if (!seen[i]) reach->lost.push_back((uint32_t)i);
            reach->strongly_connected = reach->unreachable == 0 && detail::flood(n, g.entry, rev, seen) == n;
        }
    }
    return std::string();
}

}  // namespace hgc
