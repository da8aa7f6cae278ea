// Audit of the HNSW graph the batched GPU build leaves behind, and of the walks' visited sets (test tool, not shipped;
// driven by tests/test_gpu_hnsw_graph_audit.py).
//
//   hnsw_graph_audit a            boundaries: single adds from empty, growth across 1024 / 2048, tiny and refused bulk adds,
//                                 deletes, 60 exact copies of one row, a zero row (euclidean dim 5, cosine dim 100)
//   hnsw_graph_audit b            (m, m0) = (4, 8) and (48, 64), manhattan and dot product, dim 16
//   hnsw_graph_audit c            ef_construction 64 / 128 / 256 / 512 (the four beam shapes), cosine dim 32; clones
//   hnsw_graph_audit d [n] [dim]  one bulk add of 40 000 rows of dim 64 (the 4096-node batch cap), then walks at ef = 512
//                                 whose visited log overflows
//   hnsw_graph_audit e            8 host threads walking at once, each on a scratch of its own
//
// After every mutation the program takes a CHECKPOINT: the graph arrays, the row slab and the host bookkeeping are copied
// out of the index (HnswGraphProbe, the friend hnsw_index.hpp names) and handed to hnsw_graph_check.hpp (G1 .. G9), and
//   V1  every WalkScratch of the pool is idle and its whole visited bitmap is zero.
// G9 (nothing unreachable from the entry point) is demanded where the build guarantees it -- stream a up to m0 + 1 nodes --
// and printed everywhere else; nodes without an incoming edge are refused everywhere but at m0 = 8, where they are counted.
// The first violation is printed and ends the program with status 1; otherwise one line "stream X: <checkpoints> ..." per
// index and "audit ok".
#include "../../vectorlite_amd/csrc/hnsw_index.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "hnsw_graph_check.hpp"

namespace vl {

struct HnswGraphProbe {
    template <typename T>
    static bool down(std::vector<T>& dst, const T* src, uint64_t count)
    {
        dst.resize(count);
        if (count == 0) return true;
        if (!src) return false;
        return hipMemcpy(dst.data(), src, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
    }

    static bool snapshot(const HnswIndex& ix, hgc::Graph* out)
    {
        std::shared_lock<RwLock> lk(ix.mu_);
        if (hipSetDevice(ix.device_) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
        hgc::Graph& g = *out;
        g = hgc::Graph{};
        g.n = ix.n_nodes_;
        g.m = ix.params_.m;
        g.m0 = ix.params_.m0;
        g.metric = ix.metric_;
        g.seed = ix.params_.seed;
        g.g_cap = ix.g_cap_;
        g.u_cap = ix.u_cap_;
        g.n_upper = ix.n_upper_;
        g.entry = ix.entry_;
        g.max_level = ix.max_level_;
        g.ld = g.n ? ix.store_->slab_ld() : 0;
        bool ok = true;
        ok = ok && down(g.level, ix.d_level_, g.g_cap) && down(g.upper_off, ix.d_upper_off_, g.g_cap);
        ok = ok && down(g.cnt0, ix.d_cnt0_, g.g_cap) && down(g.lock, ix.d_lock_, g.g_cap) && down(g.indeg0, ix.d_indeg0_, g.g_cap);
        ok = ok && down(g.nbr0, ix.d_nbr0_, g.n * g.m0) && down(g.dist0, reinterpret_cast<const uint64_t*>(ix.d_dist0_), g.n * g.m0);
        ok = ok && down(g.cntU, ix.d_cntU_, g.u_cap) && down(g.nbrU, ix.d_nbrU_, g.n_upper * g.m);
        ok = ok && down(g.distU, reinterpret_cast<const uint64_t*>(ix.d_distU_), g.n_upper * g.m);
        ok = ok && down(g.node_id, reinterpret_cast<const uint64_t*>(ix.d_node_id_), g.n) && down(g.live, ix.d_live_, g.n);
        ok = ok && down(g.slab, ix.store_->device_slab(), g.n * g.ld) && down(g.inv_norm, ix.store_->device_inv_norm(), g.n);
        g.h_level = ix.level_;
        g.h_upper_off = ix.upper_off_;
        g.h_node_id = ix.node_id_;
        g.h_live = ix.live_;
        g.id_to_node.assign(ix.id_to_node_.begin(), ix.id_to_node_.end());
        g.live_count = ix.live_count_;
        return ok;
    }

    // V1; *scratches gets the pool's size
    static std::string visited_sets(const HnswIndex& ix, size_t* scratches)
    {
        std::lock_guard<std::mutex> lk(ix.pool_mu_);
        *scratches = ix.pool_all_.size();
        if (ix.pool_free_.size() != ix.pool_all_.size() || ix.pool_pending_ != 0)
            return "V1: " + std::to_string(ix.pool_all_.size()) + " scratches, " + std::to_string(ix.pool_free_.size()) + " idle, " +
                   std::to_string(ix.pool_pending_) + " pending";
        std::vector<uint32_t> bits;
        for (size_t i = 0; i < ix.pool_all_.size(); ++i) {
            const WalkScratch& ws = *ix.pool_all_[i];
            if (hipStreamSynchronize(ws.stream) != hipSuccess || !down(bits, ws.d_bits, (uint64_t)ws.n_slots * ws.words)) return "V1: copy failed";
            if ((uint64_t)ws.words * 32 < ix.g_cap_) return "V1: scratch " + std::to_string(i) + " is narrower than the graph's capacity";
            for (size_t w = 0; w < bits.size(); ++w)
                if (bits[w] != 0) {
                    char buf[160];
                    snprintf(buf, sizeof buf, "V1: visited word %08x left behind (scratch %zu of %u slots, slot %zu, nodes %zu..)", bits[w], i,
                             ws.n_slots, w / ws.words, (w % ws.words) * 32);
                    return buf;
                }
        }
        return std::string();
    }
};

}  // namespace vl

using namespace vl;
using Probe = HnswGraphProbe;

namespace {

[[noreturn]] void fail(const std::string& msg)
{
    printf("%s\naudit FAILED\n", msg.c_str());
    fflush(stdout);
    exit(1);
}
#define RC(x)                                                                                               \
    do {                                                                                                    \
        const int rc_ = (x);                                                                                \
        if (rc_ != OK) fail(std::string("FAIL ") + #x + " returned " + std::to_string(rc_) + ": " + last_error()); \
    } while (0)

uint64_t splitmix(uint64_t& x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double uniform01(uint64_t& x) { return ((double)(splitmix(x) >> 11) + 0.5) * 0x1.0p-53; }
double normal(uint64_t& x) { return std::sqrt(-2.0 * std::log(uniform01(x))) * std::cos(6.283185307179586 * uniform01(x)); }

std::vector<double> gaussian_rows(uint64_t seed, uint64_t n, uint32_t dim, double scale = 1.0)
{
    uint64_t r = seed;
    std::vector<double> v(n * dim);
    for (double& x : v) x = scale * normal(r);
    return v;
}
std::vector<double> clustered_rows(uint64_t seed, uint64_t n, uint32_t dim, uint32_t clusters)
{
    uint64_t r = seed;
    const std::vector<double> centres = gaussian_rows(seed ^ 0xC0FFEEull, clusters, dim);
    std::vector<double> v(n * dim);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t c = splitmix(r) % clusters;
        for (uint32_t j = 0; j < dim; ++j) v[i * dim + j] = centres[c * dim + j] + 0.05 * normal(r);
    }
    return v;
}
uint64_t id_of(uint64_t i) { return 1000 + 3 * i; }
std::vector<uint64_t> ids_of(uint64_t first, uint64_t n)
{
    std::vector<uint64_t> v(n);
    for (uint64_t i = 0; i < n; ++i) v[i] = id_of(first + i);
    return v;
}

struct Owned {
    HnswIndex* ix = nullptr;
    ~Owned() { delete ix; }
};

HnswIndex* make(uint32_t dim, int metric, uint32_t m, uint32_t m0, uint32_t efc, uint64_t seed)
{
    HnswParams p;
    p.m = m;
    p.m0 = m0;
    p.ef_construction = efc;
    p.seed = seed;
    HnswIndex* ix = nullptr;
    RC(HnswIndex::create(dim, metric, p, 0, &ix));
    return ix;
}

struct Stream {
    std::string name;
    int checkpoints = 0;
    uint64_t worst_unreachable = 0;
    bool always_strong = true;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();

    uint64_t worst_orphans = 0;

    // the graph checker and V1 on the index as it stands; returns the snapshot.  demand_reachable: G9 must report nothing
    // unreachable; report_orphans: nodes without an incoming edge are counted, not refused (lists of 8: see DESIGN.md)
    hgc::Graph checkpoint(const HnswIndex& ix, const std::string& label, bool demand_reachable, bool report_orphans = false)
    {
        hgc::Graph g;
        if (!Probe::snapshot(ix, &g)) fail("FAIL " + name + " [" + label + "]: could not copy the graph back");
        hgc::Reach reach;
        const std::string where = name + " [" + label + ", n = " + std::to_string(g.n) + "]: ";
        const std::string v = hgc::check(g, &reach, report_orphans);
        if (!v.empty()) fail("FAIL " + where + v);
        size_t scratches = 0;
        const std::string v1 = Probe::visited_sets(ix, &scratches);
        if (!v1.empty()) fail("FAIL " + where + v1);
        if (reach.unreachable != 0 && (demand_reachable || reach.unreachable > worst_unreachable)) {
            // who they are and who names them: an island is closed under incoming edges
            std::string who;
            for (uint32_t u : reach.lost) {
                who += " " + std::to_string(u) + " (named by";
                for (uint64_t i = 0; i < g.n; ++i)
                    for (uint32_t t = 0; t < g.cnt0[i]; ++t)
                        if (g.nbr0[i * g.m0 + t] == u) who += " " + std::to_string(i);
                who += ")";
            }
            const std::string msg = where + "G9: " + std::to_string(reach.unreachable) + " nodes cannot be reached on layer 0 from the entry point:" + who;
            if (demand_reachable) fail("FAIL " + msg);
            if (reach.unreachable <= 8) printf("note %s\n", msg.c_str());
        }
        worst_unreachable = std::max(worst_unreachable, reach.unreachable);
        worst_orphans = std::max(worst_orphans, reach.orphans);
        always_strong = always_strong && reach.strongly_connected;
        ++checkpoints;
        return g;
    }
    void done(const std::string& what)
    {
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("stream %s: %d checkpoints %s unreachable_max=%llu orphans_max=%llu strongly_connected_always=%d %.2f s\n", name.c_str(), checkpoints,
               what.c_str(), (unsigned long long)worst_unreachable, (unsigned long long)worst_orphans, (int)always_strong, s);
        fflush(stdout);
    }
};

template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b, uint64_t count)
{
    return a.size() >= count && b.size() >= count && (count == 0 || std::memcmp(a.data(), b.data(), count * sizeof(T)) == 0);
}
// first array in which two snapshots differ over the nodes and slots in use ("" = none); tombstones optionally apart
std::string differs(const hgc::Graph& a, const hgc::Graph& b, bool with_live)
{
    if (a.n != b.n || a.n_upper != b.n_upper) return "n / n_upper";
    if (a.entry != b.entry || a.max_level != b.max_level || a.m != b.m || a.m0 != b.m0 || a.ld != b.ld) return "entry / max_level / m / m0 / ld";
    const uint64_t n = a.n, u = a.n_upper;
    if (!same(a.level, b.level, n)) return "level";
    if (!same(a.upper_off, b.upper_off, n)) return "upper_off";
    if (!same(a.cnt0, b.cnt0, n)) return "cnt0";
    if (!same(a.indeg0, b.indeg0, n)) return "indeg0";
    if (!same(a.lock, b.lock, n)) return "lock";
    if (!same(a.nbr0, b.nbr0, n * a.m0)) return "nbr0";
    if (!same(a.dist0, b.dist0, n * a.m0)) return "dist0";
    if (!same(a.cntU, b.cntU, u)) return "cntU";
    if (!same(a.nbrU, b.nbrU, u * a.m)) return "nbrU";
    if (!same(a.distU, b.distU, u * a.m)) return "distU";
    if (!same(a.node_id, b.node_id, n)) return "node_id";
    if (!same(a.slab, b.slab, n * a.ld)) return "slab";
    if (!same(a.inv_norm, b.inv_norm, n)) return "inv_norm";
    if (a.h_level != b.h_level || a.h_upper_off != b.h_upper_off || a.h_node_id != b.h_node_id) return "host level / upper_off / node_id";
    if (with_live) {
        if (!same(a.live, b.live, n) || a.h_live != b.h_live || a.live_count != b.live_count) return "live";
        auto x = a.id_to_node, y = b.id_to_node;
        std::sort(x.begin(), x.end());
        std::sort(y.begin(), y.end());
        if (x != y) return "id_to_node";
    }
    return std::string();
}

// ---------------------------------------------------------------------------------------------------------------------
void stream_a()
{
    const struct {
        uint32_t dim;
        int metric;
    } cfg[2] = {{5, EUCLIDEAN}, {100, COSINE}};
    for (const auto& c : cfg) {
        Stream st;
        st.name = "a";
        Owned o;
        o.ix = make(c.dim, c.metric, 16, 32, 32, 11);
        HnswIndex& ix = *o.ix;
        const uint32_t dim = c.dim;
        const uint64_t total = 2100;
        std::vector<double> rows = gaussian_rows(0xA000 + dim, total, dim);
        for (uint32_t j = 0; j < dim; ++j) rows[7 * dim + j] = 0.0;  // a zero row (no direction under cosine)
        for (uint64_t i = 21; i < 24; ++i) std::memcpy(&rows[i * dim], &rows[20 * dim], dim * sizeof(double));     // copies among the single adds
        for (uint64_t i = 101; i < 160; ++i) std::memcpy(&rows[i * dim], &rows[100 * dim], dim * sizeof(double));  // 60 copies of one row
        for (uint32_t j = 0; j < dim; ++j) rows[1500 * dim + j] = 0.0;
        uint64_t n = 0;
        // Up to m0 + 1 nodes no list is ever full: every link is made both ways and nothing is evicted, so everything is
        // reachable from everything.  Beyond that the build promises every node an incoming edge (G6), not a path from the
        // entry point: the count is printed with the nodes and who names them.
        auto must_reach = [&]() { return n <= 33; };
        auto add = [&](uint64_t count, const char* what) {
            const std::vector<uint64_t> ids = ids_of(n, count);
            RC(ix.add_bulk(ids.data(), &rows[n * dim], count, false));
            n += count;
            return st.checkpoint(ix, std::string(what) + " to " + std::to_string(n), must_reach());
        };
        (void)st.checkpoint(ix, "empty", true);
        for (int i = 0; i < 40; ++i) {  // first node, first link, first full list and eviction at n = 33 / 34
            const uint64_t id = id_of(n);
            RC(ix.add(id, &rows[n * dim], dim));
            ++n;
            (void)st.checkpoint(ix, "single add to " + std::to_string(n), must_reach());
        }
        (void)add(1030 - n, "bulk add");  // across the capacity of 1024: every array regrown, the scratch pool dropped
        (void)add(2060 - n, "bulk add");  // across 2048
        (void)add(1, "bulk add of 1");
        (void)add(2, "bulk add of 2");
        hgc::Graph before = add(17, "bulk add of 17");
        {  // refused at position 0: nothing is added
            std::vector<uint64_t> ids = ids_of(n, 6);
            ids[0] = id_of(5);
            const int rc = ix.add_bulk(ids.data(), &rows[n * dim], 6, false);
            if (rc != ERR_DUP_ID) fail("FAIL a: a bulk add whose first id exists returned " + std::to_string(rc));
            const hgc::Graph after = st.checkpoint(ix, "refused bulk add (position 0)", false);
            const std::string d = differs(before, after, true);
            if (!d.empty()) fail("FAIL a: a bulk add refused at position 0 changed " + d);
        }
        {  // refused at position 3: the first three rows are in, as if they had been added alone
            std::vector<uint64_t> ids = ids_of(n, 6);
            ids[3] = ids[1];
            const int rc = ix.add_bulk(ids.data(), &rows[n * dim], 6, false);
            if (rc != ERR_DUP_ID) fail("FAIL a: a bulk add whose fourth id repeats returned " + std::to_string(rc));
            const hgc::Graph after = st.checkpoint(ix, "refused bulk add (position 3)", false);
            if (after.n != n + 3 || ix.len() != n + 3) fail("FAIL a: a bulk add refused at position 3 left " + std::to_string(after.n) + " nodes, not n + 3");
            for (uint64_t i = 0; i < 3; ++i) {
                if (after.h_node_id[n + i] != ids[i]) fail("FAIL a: refused bulk add: wrong id at node " + std::to_string(n + i));
                for (uint32_t j = 0; j < dim; ++j)
                    if (after.slab[(n + i) * after.ld + j] != (float)rows[(n + i) * dim + j]) fail("FAIL a: refused bulk add: wrong row at node " + std::to_string(n + i));
            }
            // the nodes that were there keep everything but the lists the three new nodes linked into
            if (!same(before.level, after.level, n) || !same(before.upper_off, after.upper_off, n) || !same(before.node_id, after.node_id, n) ||
                !same(before.slab, after.slab, n * after.ld))
                fail("FAIL a: a bulk add refused at position 3 changed an earlier node's level, offset, id or row");
            n += 3;
            before = after;
        }
        const uint64_t doomed[10] = {0, 1, n - 1, 7, 100, 130, 1023, 1024, 2047, 2048};  // the first entry point, edges of the capacity steps, copies
        for (int i = 0; i < 10; ++i) {  // tombstones only: every byte but `live` stays
            RC(ix.remove(id_of(doomed[i])));
            const hgc::Graph after = st.checkpoint(ix, "delete of node " + std::to_string(doomed[i]), false);
            const std::string d = differs(before, after, false);
            if (!d.empty()) fail("FAIL a: a delete changed " + d);
            if (after.h_live[doomed[i]] != 0 || after.live_count + 1 != before.live_count) fail("FAIL a: a delete did not tombstone its node");
            before = after;
        }
        if (ix.remove(id_of(0)) != ERR_NOT_FOUND) fail("FAIL a: a second delete of one id was accepted");
        st.done("dim=" + std::to_string(dim) + " metric=" + std::to_string(c.metric) + " n=" + std::to_string(n));
    }
}

void stream_b()
{
    const struct {
        uint32_t m, m0;
        uint64_t n;
        uint64_t pieces[5];
    } shape[2] = {{4, 8, 2000, {1, 199, 300, 700, 800}}, {48, 64, 600, {1, 59, 140, 150, 250}}};
    const int metrics[2] = {MANHATTAN, DOT};
    const uint32_t dim = 16;
    for (const auto& s : shape)
        for (int metric : metrics) {
            Stream st;
            st.name = "b";
            Owned o;
            o.ix = make(dim, metric, s.m, s.m0, 32, 23);
            // (4, 8): 20 tight clusters, so every list is fought over; (48, 64): lists longer than one round of 32 lanes
            const std::vector<double> rows = s.m == 4 ? clustered_rows(0xB000 + metric, s.n, dim, 20) : gaussian_rows(0xB100 + metric, s.n, dim);
            uint64_t n = 0;
            uint32_t longest = 0;
            for (uint64_t piece : s.pieces) {
                const std::vector<uint64_t> ids = ids_of(n, piece);
                RC(o.ix->add_bulk(ids.data(), &rows[n * dim], piece, false));
                n += piece;
                const hgc::Graph g = st.checkpoint(*o.ix, "bulk add to " + std::to_string(n), false, /*report_orphans=*/s.m0 == 8);
                for (uint64_t i = 0; i < g.n; ++i) longest = std::max(longest, g.cnt0[i]);
            }
            if (s.m0 == 64 && longest <= 32) fail("FAIL b: no layer-0 list grew past 32 entries at m0 = 64");
            st.done("m=" + std::to_string(s.m) + " m0=" + std::to_string(s.m0) + " metric=" + std::to_string(metric) + " n=" + std::to_string(n) +
                    " longest_list=" + std::to_string(longest));
        }
}

HnswIndex* build_c(uint32_t efc, std::vector<double>* rows_out)
{
    const uint32_t dim = 32;
    const uint64_t n = 3000;
    HnswIndex* ix = make(dim, COSINE, 16, 32, efc, 31);
    std::vector<double> rows = gaussian_rows(0xC000, n + 50, dim);
    const std::vector<uint64_t> ids = ids_of(0, n);
    RC(ix->add_bulk(ids.data(), rows.data(), n, false));
    if (rows_out) *rows_out = std::move(rows);
    return ix;
}

void stream_c()
{
    const uint32_t dim = 32;
    const uint64_t n = 3000;
    for (uint32_t efc : {64u, 128u, 256u, 512u}) {
        Stream st;
        st.name = "c";
        std::vector<double> rows;
        Owned src, cl;
        src.ix = build_c(efc, &rows);
        const hgc::Graph g0 = st.checkpoint(*src.ix, "bulk add to 3000", false);
        RC(src.ix->clone(&cl.ix));
        const hgc::Graph gc = st.checkpoint(*cl.ix, "clone", false);  // G7 on the clone's own tails among the rest
        std::string d = differs(g0, gc, true);
        if (!d.empty()) fail("FAIL c: the clone differs from its source in " + d);
        const std::vector<uint64_t> ids = ids_of(n, 50);
        RC(cl.ix->add_bulk(ids.data(), &rows[n * dim], 50, false));
        const hgc::Graph gc2 = st.checkpoint(*cl.ix, "clone + 50", false);
        if (gc2.n != n + 50) fail("FAIL c: the clone did not take 50 rows");
        const hgc::Graph g1 = st.checkpoint(*src.ix, "source after the clone grew", false);
        d = differs(g0, g1, true);
        if (!d.empty()) fail("FAIL c: adding to the clone moved the source's " + d);
        st.done("ef_construction=" + std::to_string(efc) + " n=" + std::to_string(n));
    }
}

struct Answer {
    std::vector<uint64_t> ids, n;
    std::vector<double> scores;
    bool operator==(const Answer& o) const
    {
        return ids == o.ids && n == o.n && scores.size() == o.scores.size() &&
               (scores.empty() || std::memcmp(scores.data(), o.scores.data(), scores.size() * sizeof(double)) == 0);
    }
};
Answer walk(const HnswIndex& ix, const double* q, uint64_t nq, uint32_t dim, uint64_t k, uint32_t ef, bool single)
{
    Answer a;
    a.ids.assign(nq * k, 0);
    a.scores.assign(nq * k, 0.0);
    a.n.assign(nq, 0);
    if (single)
        RC(ix.search(q, dim, k, ix.metric(), ef, a.ids.data(), a.scores.data(), a.n.data()));
    else
        RC(ix.search_batch(q, nq, dim, k, ix.metric(), ef, a.ids.data(), a.scores.data(), a.n.data()));
    return a;
}

void stream_d(uint64_t n, uint32_t dim)
{
    Stream st;
    st.name = "d";
    Owned o;
    o.ix = make(dim, EUCLIDEAN, 16, 32, 32, 41);
    {
        uint64_t r = 0xD000;
        std::vector<double> rows(n * dim);
        for (double& x : rows) x = uniform01(r);
        const std::vector<uint64_t> ids = ids_of(0, n);
        RC(o.ix->add_bulk(ids.data(), rows.data(), n, false));  // one call: batches reach the cap of 4096 nodes
    }
    (void)st.checkpoint(*o.ix, "bulk add to " + std::to_string(n), false);
    const uint64_t nq = 64, k = 100;
    uint64_t r = 0xD111;
    std::vector<double> q(nq * dim);
    for (double& x : q) x = uniform01(r);
    uint64_t e0 = 0, e1 = 0, e2 = 0;
    o.ix->walk_stats(nullptr, &e0);
    const Answer a1 = walk(*o.ix, q.data(), nq, dim, k, 512, false);
    o.ix->walk_stats(nullptr, &e1);
    (void)st.checkpoint(*o.ix, "first batch at ef = 512", false);
    const Answer a2 = walk(*o.ix, q.data(), nq, dim, k, 512, false);
    o.ix->walk_stats(nullptr, &e2);
    (void)st.checkpoint(*o.ix, "second batch at ef = 512", false);
    const double per_query = (double)(e1 - e0) / (double)nq;
    printf("d: n=%llu dim=%u evaluations per query: %.1f (first batch), %.1f (second)\n", (unsigned long long)n, dim, per_query,
           (double)(e2 - e1) / (double)nq);
    // a walk's evaluations are the nodes it marked + the entry point + the 512 exact re-scorings of its beam: more than
    // 8192 + 513 on average means the average walk marked more than WALK_LOG_CAP = 8192 nodes and wiped its whole bitmap
    if (!(per_query > 8192.0)) fail("FAIL d: the walks do not overflow the visited log: " + std::to_string(per_query) + " evaluations per query");
    if (!(per_query > 8192.0 + 513.0)) fail("FAIL d: the walks mark fewer than 8192 nodes on average: " + std::to_string(per_query) + " evaluations per query");
    if (e2 - e1 != e1 - e0) fail("FAIL d: the same batch made " + std::to_string(e1 - e0) + " evaluations, then " + std::to_string(e2 - e1));
    if (!(a1 == a2)) fail("FAIL d: the same batch returned different ids or score bits the second time");
    for (uint64_t i = 0; i < nq; ++i)
        if (a1.n[i] != k) fail("FAIL d: a query returned " + std::to_string(a1.n[i]) + " results");
    char buf[96];
    snprintf(buf, sizeof buf, "n=%llu dim=%u evals_per_query=%.1f", (unsigned long long)n, dim, per_query);
    st.done(buf);
}

void stream_e()
{
    Stream st;
    st.name = "e";
    const uint32_t dim = 32;
    Owned o;
    o.ix = build_c(128, nullptr);
    HnswIndex& ix = *o.ix;
    ix.set_coalescing(0, 0);  // every caller walks alone, on a scratch of its own
    (void)st.checkpoint(ix, "bulk add to 3000", false);
    constexpr int THREADS = 8, SINGLES = 20, BATCHES = 5, NB = 100;
    const uint64_t k = 10;
    const std::vector<double> q = gaussian_rows(0xE000, (uint64_t)THREADS * (SINGLES + BATCHES * NB), dim);
    std::vector<std::vector<Answer>> got(THREADS);
    auto calls = [&](int t, std::vector<Answer>& out) {
        const double* base = &q[(uint64_t)t * (SINGLES + BATCHES * NB) * dim];
        for (int i = 0; i < SINGLES; ++i) out.push_back(walk(ix, base + (uint64_t)i * dim, 1, dim, k, i % 2 ? 200 : 10, true));
        for (int b = 0; b < BATCHES; ++b) out.push_back(walk(ix, base + (uint64_t)(SINGLES + b * NB) * dim, NB, dim, k, b % 2 ? 10 : 200, false));
    };
    {
        std::vector<std::thread> th;
        for (int t = 0; t < THREADS; ++t) th.emplace_back([&, t]() { calls(t, got[t]); });
        for (auto& x : th) x.join();
    }
    size_t scratches = 0;
    (void)Probe::visited_sets(ix, &scratches);
    (void)st.checkpoint(ix, "after 8 threads", false);
    for (int t = 0; t < THREADS; ++t) {
        std::vector<Answer> alone;
        calls(t, alone);
        for (size_t i = 0; i < alone.size(); ++i)
            if (!(alone[i] == got[t][i])) fail("FAIL e: thread " + std::to_string(t) + " call " + std::to_string(i) + " was answered differently among 7 others than alone");
    }
    (void)st.checkpoint(ix, "after the replays", false);
    st.done("threads=8 scratches=" + std::to_string(scratches));
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string which = argc > 1 ? argv[1] : "";
    if (which == "a") stream_a();
    else if (which == "b") stream_b();
    else if (which == "c") stream_c();
    else if (which == "d") stream_d(argc > 2 ? strtoull(argv[2], nullptr, 10) : 40000, argc > 3 ? (uint32_t)atoi(argv[3]) : 64);
    else if (which == "e") stream_e();
    else {
        printf("usage: hnsw_graph_audit a|b|c|d [n] [dim]|e\n");
        return 2;
    }
    printf("audit ok\n");
    return 0;
}
