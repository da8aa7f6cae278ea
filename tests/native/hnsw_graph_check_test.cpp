// hnsw_graph_check.hpp on the CPU (stand-alone, run under ASan + UBSan by tests/test_hnsw_graph_check_cpu.py):
//   - the level law against values worked out by hand (splitmix64 in integer arithmetic, then the logarithms);
//   - the f32 edge key against a long-double evaluation of the same distance (a wrong chunk order or tail shows as a
//     difference far above f32 rounding; agreement within 1e-5 of the scaled distance is all that is asked);
//   - a correct 12-node, two-layer, dim-5 graph passes under all four metrics;
//   - every invariant G1 .. G8 broken alone is named, and only it.
#include "hnsw_graph_check.hpp"

#include <cstdio>
#include <cstdlib>
#include <functional>

using namespace hgc;

namespace {
int failures = 0;
#define EXPECT(cond, ...)                                    \
    do {                                                     \
        if (!(cond)) {                                       \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);      \
            printf(__VA_ARGS__);                             \
            printf("\n");                                    \
            ++failures;                                      \
        }                                                    \
    } while (0)

uint64_t rng_state = 12345;
double uniform()
{
    rng_state = splitmix64(rng_state);
    return ((double)(rng_state >> 11) + 0.5) * 0x1.0p-53;
}

// seed 2, m = 4 puts nodes 0, 3 and 8 on level 1 and every other of the first twelve on level 0
constexpr uint64_t SEED = 2;
constexpr uint32_t N = 12, M = 4, M0 = 6, DIM = 5, LD = 8;

void set_distances(Graph& g)
{
    for (uint64_t i = 0; i < g.n; ++i)
        for (int layer = 0; layer <= (int)g.level[i]; ++layer) {
            const uint64_t slot = layer == 0 ? i : g.upper_off[i] + (uint64_t)(layer - 1);
            const uint32_t cnt = layer == 0 ? g.cnt0[i] : g.cntU[slot];
            for (uint32_t t = 0; t < cnt; ++t) {
                const uint32_t v = layer == 0 ? g.nbr0[i * g.m0 + t] : g.nbrU[slot * g.m + t];
                const uint64_t a = i > v ? i : v, b = i > v ? v : i;
                const uint64_t key = edge_key_f32(g.metric, &g.slab[a * g.ld], g.inv_norm[a], &g.slab[b * g.ld], g.inv_norm[b], g.ld);
                (layer == 0 ? g.dist0[i * g.m0 + t] : g.distU[slot * g.m + t]) = key;
            }
        }
}

Graph hand_graph(int metric)
{
    Graph g;
    g.n = N;
    g.m = M;
    g.m0 = M0;
    g.metric = metric;
    g.ld = LD;
    g.seed = SEED;
    g.g_cap = 16;
    g.u_cap = 4;
    g.level.assign(g.g_cap, 0);
    g.upper_off.assign(g.g_cap, 0);
    g.cnt0.assign(g.g_cap, 0);
    g.lock.assign(g.g_cap, 0);
    g.indeg0.assign(g.g_cap, 0);
    g.cntU.assign(g.u_cap, 0);
    const int levels[N] = {1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0};
    uint32_t run = 0;
    for (uint32_t i = 0; i < N; ++i) {
        g.level[i] = (uint8_t)levels[i];
        g.upper_off[i] = run;
        run += (uint32_t)levels[i];
    }
    g.n_upper = run;
    g.entry = 0;
    g.max_level = 1;
    g.h_level.assign(g.level.begin(), g.level.begin() + N);
    g.h_upper_off.assign(g.upper_off.begin(), g.upper_off.begin() + N);
    g.slab.assign((size_t)N * LD, 0.f);
    g.inv_norm.assign(N, 0.f);
    rng_state = 99;
    for (uint32_t i = 0; i < N; ++i) {
        float ss = 0.f;
        for (uint32_t c = 0; c < DIM; ++c) {
            const float v = (float)(2.0 * uniform() - 1.0);
            g.slab[(size_t)i * LD + c] = v;
            ss += v * v;
        }
        g.inv_norm[i] = 1.0f / sqrtf(ss);
    }
    // layer 0: a ring, every node lists i +- 1 and i +- 2; layer 1: nodes 0, 3, 8 list each other
    g.nbr0.assign((size_t)N * M0, 0xDDDDDDDDu);
    g.dist0.assign((size_t)N * M0, 0xDDDDDDDDDDDDDDDDull);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t nb[4] = {(i + 1) % N, (i + N - 1) % N, (i + 2) % N, (i + N - 2) % N};
        for (int t = 0; t < 4; ++t) g.nbr0[(size_t)i * M0 + t] = nb[t];
        g.cnt0[i] = 4;
        g.indeg0[i] = 4;
    }
    g.nbrU.assign((size_t)g.n_upper * M, 0xDDDDDDDDu);
    g.distU.assign((size_t)g.n_upper * M, 0xDDDDDDDDDDDDDDDDull);
    const uint32_t up[3] = {0, 3, 8};
    for (uint32_t a = 0; a < 3; ++a) {
        uint32_t t = 0;
        for (uint32_t b = 0; b < 3; ++b)
            if (b != a) g.nbrU[(size_t)a * M + t++] = up[b];
        g.cntU[a] = 2;
    }
    set_distances(g);
    g.node_id.resize(N);
    g.live.assign(N, 1);
    for (uint32_t i = 0; i < N; ++i) {
        g.node_id[i] = 1000 + 7 * (uint64_t)i;
        g.id_to_node.push_back({g.node_id[i], i});
    }
    g.h_node_id = g.node_id;
    g.h_live = g.live;
    g.live_count = N;
    return g;
}

void expect_named(const char* inv, const char* what, const std::function<void(Graph&)>& breakit)
{
    Graph g = hand_graph(EUCLIDEAN);
    breakit(g);
    const std::string v = check(g);
    EXPECT(v.compare(0, 3, std::string(inv) + ":") == 0, "%s (%s): the checker said \"%s\"", inv, what, v.c_str());
}

long double exact_scaled(int metric, const float* q, const float* r, uint32_t dim)
{
    long double dot = 0, qq = 0, rr = 0, l2 = 0, l1 = 0;
    for (uint32_t c = 0; c < dim; ++c) {
        const long double a = q[c], b = r[c];
        dot += a * b;
        qq += a * a;
        rr += b * b;
        l2 += (a - b) * (a - b);
        l1 += fabsl(a - b);
    }
    if (metric == COSINE) return (1.0L - dot / (sqrtl(qq) * sqrtl(rr))) * 1000.0L;
    if (metric == EUCLIDEAN) return sqrtl(l2) * 1000.0L;
    if (metric == MANHATTAN) return l1 * 1000.0L;
    return 1000.0L - dot;
}
}  // namespace

int main()
{
    // ---- the level law.  splitmix64(0) = e220a8397b1dcdaf (the published first output of the generator), so
    // u = (0xe220a8397b1dcdaf >> 11 + 1) / 2^53 = 0.8833..., -ln u = 0.124: level 0 for every m >= 2.
    EXPECT(splitmix64(0) == 0xe220a8397b1dcdafull, "splitmix64(0)");
    EXPECT(level_law(0, 0, 16) == 0, "level(0, 0, 16)");
    // worked out with integer arithmetic and logarithms outside this program
    EXPECT(level_law(5, 7, 4) == 3, "level(5, 7, 4) = %d", level_law(5, 7, 4));
    EXPECT(level_law(5, 9, 4) == 1, "level(5, 9, 4) = %d", level_law(5, 9, 4));
    EXPECT(level_law(5, 10, 4) == 5, "level(5, 10, 4) = %d", level_law(5, 10, 4));
    EXPECT(level_law(0, 558, 16) == 2, "level(0, 558, 16) = %d", level_law(0, 558, 16));
    EXPECT(level_law(0, 557, 16) == 0, "level(0, 557, 16) = %d", level_law(0, 557, 16));
    EXPECT(level_law(3, 77, 2) == 1, "level(3, 77, 2) = %d", level_law(3, 77, 2));
    EXPECT(level_law(0xDEADBEEFull, 99, 4) == 0, "level(0xDEADBEEF, 99, 4)");
    EXPECT(level_law(1, (1ull << 32) + 5, 48) == 0, "level(1, 2^32 + 5, 48)");
    {
        const int want[12] = {1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0};
        for (int i = 0; i < 12; ++i) EXPECT(level_law(SEED, (uint64_t)i, M) == want[i], "level(2, %d, 4)", i);
    }

    // ---- the f32 key against long double, at the dims whose chunk counts differ in parity and length
    for (uint32_t dim : {1u, 5u, 8u, 16u, 100u, 384u, 387u}) {
        const uint32_t ld = (dim + 3) & ~3u;
        std::vector<float> q(ld, 0.f), r(ld, 0.f);
        for (int rep = 0; rep < 20; ++rep) {
            float qq = 0.f, rr = 0.f;
            for (uint32_t c = 0; c < dim; ++c) {
                q[c] = (float)(2.0 * uniform() - 1.0);
                r[c] = (float)(2.0 * uniform() - 1.0);
                qq += q[c] * q[c];
                rr += r[c] * r[c];
            }
            for (int metric = 0; metric < 4; ++metric) {
                const uint64_t key = edge_key_f32(metric, q.data(), 1.0f / sqrtf(qq), r.data(), 1.0f / sqrtf(rr), ld);
                double got;
                std::memcpy(&got, &key, sizeof got);
                const long double want = exact_scaled(metric, q.data(), r.data(), dim);
                // 1e-5 of the scaled distance; the cosine tail rounds a similarity near 1 to f32 before it subtracts, which
                // alone is worth a few units of 2^-24 of the 1000 it is scaled by, however small the distance
                const long double bound = 1e-5L * fabsl(want) + (metric == COSINE ? 1000.0L * 4.0L * 0x1.0p-24L : 0.0L);
                EXPECT(fabsl((long double)got - want) <= bound, "f32 key, metric %d dim %u: %.9g against %.9Lg", metric, dim, got, want);
            }
        }
    }
    {
        const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8] = {1, 2, 3, 4, 5, 0, 0, 0};
        double d;
        uint64_t key = edge_key_f32(COSINE, o, 0.1f, z, 0.f, 8);  // a zero row under cosine: the reference's `return 1000`
        std::memcpy(&d, &key, sizeof d);
        EXPECT(d == 1000.0, "cosine with a zero row: %g", d);
        EXPECT(edge_key_f32(EUCLIDEAN, o, 0.f, o, 0.f, 8) == 0, "a row against itself");
        EXPECT(walk_key(-1.0) == 0 && walk_key(0.0) == 0 && walk_key(std::nan("")) == 0, "walk_key clamps");
    }

    // ---- the correct graph
    for (int metric = 0; metric < 4; ++metric) {
        const Graph g = hand_graph(metric);
        Reach r;
        const std::string v = check(g, &r);
        EXPECT(v.empty(), "the correct graph, metric %d: \"%s\"", metric, v.c_str());
        EXPECT(r.unreachable == 0 && r.strongly_connected, "the ring is strongly connected");
    }
    {  // G9 on one-way graphs
        Reach r;
        Graph g = hand_graph(EUCLIDEAN);
        // a one-way graph: 0 -> 1 -> ... -> 11, nothing back: all reachable from the entry point, not strongly connected
        for (uint32_t i = 0; i < N; ++i) {
            g.cnt0[i] = i + 1 < N ? 1 : 0;
            g.nbr0[(size_t)i * M0] = i + 1;
            g.indeg0[i] = i > 0 ? 1 : 0;
        }
        set_distances(g);
        std::string v = check(g, &r);
        EXPECT(v.compare(0, 3, "G6:") == 0, "node 0 of the chain has no incoming edge: \"%s\"", v.c_str());
        g.cnt0[N - 1] = 1;  // close the chain into a cycle
        g.nbr0[(size_t)(N - 1) * M0] = 0;
        g.indeg0[0] = 1;
        set_distances(g);
        v = check(g, &r);
        EXPECT(v.empty() && r.unreachable == 0 && r.strongly_connected, "the cycle: \"%s\"", v.c_str());
        // two cycles 0..5 and 6..11 with one edge 5 -> 6 across: everything reachable from 0, nothing comes back
        g.nbr0[(size_t)5 * M0 + 1] = 6;
        g.cnt0[5] = 2;
        g.nbr0[(size_t)5 * M0] = 0;
        g.nbr0[(size_t)11 * M0] = 6;
        g.indeg0[6] = 2;
        set_distances(g);
        v = check(g, &r);
        EXPECT(v.empty() && r.unreachable == 0 && !r.strongly_connected, "one-way bridge: \"%s\" %llu", v.c_str(), (unsigned long long)r.unreachable);
        // the bridge the other way round: 6..11 cannot be reached from the entry point
        g.cnt0[5] = 1;
        g.indeg0[6] = 1;
        g.nbr0[(size_t)11 * M0 + 1] = 0;
        g.cnt0[11] = 2;
        g.nbr0[(size_t)11 * M0] = 6;
        g.indeg0[0] = 2;
        set_distances(g);
        v = check(g, &r);
        EXPECT(v.empty() && r.unreachable == 6 && !r.strongly_connected, "unreachable half: \"%s\" %llu", v.c_str(), (unsigned long long)r.unreachable);
    }

    // ---- one invariant broken at a time
    expect_named("G1", "device level", [](Graph& g) { g.level[4] = 1; });
    expect_named("G1", "host level", [](Graph& g) { g.h_level[3] = 0; });
    expect_named("G1", "device upper_off", [](Graph& g) { g.upper_off[5] = 1; });
    expect_named("G1", "host upper_off", [](Graph& g) { g.h_upper_off[11] = 2; });
    expect_named("G1", "n_upper", [](Graph& g) { g.n_upper = 4; });
    expect_named("G1", "g_cap", [](Graph& g) { g.g_cap = 11; });
    expect_named("G1", "u_cap", [](Graph& g) { g.u_cap = 2; });
    expect_named("G1", "another seed", [](Graph& g) { g.seed = 3; });
    expect_named("G2", "max_level", [](Graph& g) { g.max_level = 2; });
    expect_named("G2", "entry is a later node of the top level", [](Graph& g) { g.entry = 3; });
    expect_named("G2", "entry is a level-0 node", [](Graph& g) { g.entry = 1; });
    expect_named("G3", "cnt0 > m0", [](Graph& g) { g.cnt0[2] = M0 + 1; });
    expect_named("G3", "cntU > m", [](Graph& g) { g.cntU[1] = M + 1; });
    expect_named("G3", "neighbour >= n", [](Graph& g) { g.nbr0[(size_t)7 * M0 + 3] = N; });
    expect_named("G3", "uninitialised slot counted", [](Graph& g) { g.cnt0[7] = 5; });
    expect_named("G3", "self", [](Graph& g) { g.nbr0[(size_t)6 * M0 + 0] = 6; });
    expect_named("G3", "level-0 node in a layer-1 list", [](Graph& g) { g.nbrU[(size_t)2 * M + 1] = 4; });
    expect_named("G4", "layer 0", [](Graph& g) { g.nbr0[(size_t)9 * M0 + 2] = g.nbr0[(size_t)9 * M0 + 0]; });
    expect_named("G4", "layer 1", [](Graph& g) { g.nbrU[(size_t)0 * M + 1] = g.nbrU[(size_t)0 * M + 0]; });
    expect_named("G4", "a fifth entry that repeats the first, everything else consistent", [](Graph& g) {
        g.nbr0[(size_t)9 * M0 + 4] = g.nbr0[(size_t)9 * M0 + 0];
        g.dist0[(size_t)9 * M0 + 4] = g.dist0[(size_t)9 * M0 + 0];
        g.cnt0[9] = 5;
        g.indeg0[g.nbr0[(size_t)9 * M0 + 0]] += 1;
    });
    expect_named("G5", "one bit of a layer-0 distance", [](Graph& g) { g.dist0[(size_t)3 * M0 + 2] ^= 1ull; });
    expect_named("G5", "one bit of a layer-1 distance", [](Graph& g) { g.distU[(size_t)1 * M + 0] ^= 1ull << 40; });
    expect_named("G5", "the distance of another edge of the same list", [](Graph& g) { g.dist0[(size_t)3 * M0 + 0] = g.dist0[(size_t)3 * M0 + 1]; });
    expect_named("G5", "the roles of the two rows swapped under cosine would pass; a neighbour swap does not", [](Graph& g) {
        std::swap(g.nbr0[(size_t)4 * M0 + 0], g.nbr0[(size_t)4 * M0 + 2]);
    });
    expect_named("G6", "indeg0 one too many", [](Graph& g) { g.indeg0[10] += 1; });
    expect_named("G6", "indeg0 one too few", [](Graph& g) { g.indeg0[0] -= 1; });
    expect_named("G6", "an entry dropped without its count", [](Graph& g) { g.cnt0[1] = 3; });
    expect_named("G7", "lock inside n", [](Graph& g) { g.lock[5] = 1; });
    expect_named("G7", "lock beyond n", [](Graph& g) { g.lock[15] = 1; });
    expect_named("G7", "cnt0 beyond n", [](Graph& g) { g.cnt0[12] = 1; });
    expect_named("G7", "indeg0 beyond n", [](Graph& g) { g.indeg0[14] = 2; });
    expect_named("G7", "cntU beyond n_upper", [](Graph& g) { g.cntU[3] = 1; });
    expect_named("G8", "device live", [](Graph& g) { g.live[2] = 0; });
    expect_named("G8", "device node_id", [](Graph& g) { g.node_id[2] += 1; });
    expect_named("G8", "live_count", [](Graph& g) { g.live_count -= 1; });
    expect_named("G8", "a tombstone still in id_to_node", [](Graph& g) {
        g.live[6] = g.h_live[6] = 0;
        g.live_count -= 1;
    });
    expect_named("G8", "id_to_node names the wrong node", [](Graph& g) { std::swap(g.id_to_node[1].second, g.id_to_node[2].second); });
    {  // a clean tombstone passes
        Graph g = hand_graph(EUCLIDEAN);
        g.live[6] = g.h_live[6] = 0;
        g.live_count -= 1;
        g.id_to_node.erase(g.id_to_node.begin() + 6);
        const std::string v = check(g);
        EXPECT(v.empty(), "a tombstone: \"%s\"", v.c_str());
    }
    {  // the empty graph and the single node
        Graph g;
        EXPECT(check(g).empty(), "the empty graph: \"%s\"", check(g).c_str());
        g = hand_graph(EUCLIDEAN);
        g.n = 1;
        g.n_upper = 1;
        g.h_level.resize(1);
        g.h_upper_off.resize(1);
        g.h_node_id.resize(1);
        g.h_live.resize(1);
        g.id_to_node.resize(1);
        g.live_count = 1;
        for (uint32_t i = 0; i < 16; ++i) g.cnt0[i] = g.indeg0[i] = 0;
        for (uint32_t s = 0; s < 4; ++s) g.cntU[s] = 0;
        EXPECT(check(g).empty(), "a single node: \"%s\"", check(g).c_str());
    }

    if (failures) {
        printf("hnsw graph check FAILED (%d)\n", failures);
        return 1;
    }
    printf("hnsw graph check ok\n");
    return 0;
}
