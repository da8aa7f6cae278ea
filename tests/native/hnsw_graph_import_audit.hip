// Audit of HnswIndex::graph_import (test tool, not shipped; driven by tests/test_gpu_hnsw_graph_import_audit.py).
//
//   hnsw_graph_import_audit a   n = 2060 (both capacity steps), euclidean dim 5 and cosine dim 100, ten tombstones, zero rows
//                               and 60 copies of one row among the data
//   hnsw_graph_import_audit b   (m, m0) = (4, 8) with manhattan and (48, 64) with the dot product, n = 600, dim 16
//   hnsw_graph_import_audit c   dim 3072, n = 300: the widest slab stride the distance routine serves
//
// Each index is built by the batched GPU build, exported (graph_export), and imported into a fresh HnswIndex.  The
// imported index's arrays are copied back (HnswGraphProbe, the friend hnsw_index.hpp names) and
//   - hnsw_graph_check.hpp (G1 .. G9) is clean on them with the source's orphan policy;
//   - level, upper_off, cnt0, nbr0, dist0, cntU, nbrU, distU, indeg0, lock, node_id, live, the slab and the host
//     bookkeeping are BITWISE equal to the source index's over the nodes and slots in use: dist0 / distU and indeg0 are what
//     the import's two kernels recompute;
//   - the orphan count the import reports is the number of nodes whose in-degree is zero;
//   - then a bulk add of 17 rows, a single add and three deletes run on the imported index, each followed by the checker.
// The first violation is printed and ends the program with status 1; otherwise one line "stream X: ..." per index and
// "audit ok".
#include "../../vectorlite_amd/csrc/hnsw_index.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
std::vector<double> gaussian_rows(uint64_t seed, uint64_t n, uint32_t dim)
{
    uint64_t r = seed;
    std::vector<double> v(n * dim);
    for (double& x : v) x = normal(r);
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
HnswIndex* make(uint32_t dim, int metric, const HnswParams& p)
{
    HnswIndex* ix = nullptr;
    RC(HnswIndex::create(dim, metric, p, 0, &ix));
    return ix;
}

template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b, uint64_t count)
{
    return a.size() >= count && b.size() >= count && (count == 0 || std::memcmp(a.data(), b.data(), count * sizeof(T)) == 0);
}
// first array in which two snapshots differ over the nodes and slots in use ("" = none)
std::string differs(const hgc::Graph& a, const hgc::Graph& b)
{
    if (a.n != b.n || a.n_upper != b.n_upper) return "n / n_upper";
    if (a.entry != b.entry || a.max_level != b.max_level || a.m != b.m || a.m0 != b.m0 || a.ld != b.ld) return "entry / max_level / m / m0 / ld";
    const uint64_t n = a.n, u = a.n_upper;
    if (!same(a.level, b.level, n)) return "level";
    if (!same(a.upper_off, b.upper_off, n)) return "upper_off";
    if (!same(a.cnt0, b.cnt0, n)) return "cnt0";
    if (!same(a.nbr0, b.nbr0, n * a.m0)) return "nbr0";
    if (!same(a.cntU, b.cntU, u)) return "cntU";
    if (!same(a.nbrU, b.nbrU, u * a.m)) return "nbrU";
    if (!same(a.slab, b.slab, n * a.ld)) return "slab";
    if (!same(a.inv_norm, b.inv_norm, n)) return "inv_norm";
    // the distances of the entries in use (what lies behind a list's count is never read: the build leaves whatever was
    // there, the import computes nothing for it)
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t t = 0; t < a.cnt0[i]; ++t)
            if (a.dist0[i * a.m0 + t] != b.dist0[i * a.m0 + t]) return "dist0 (node " + std::to_string(i) + ", slot " + std::to_string(t) + ")";
    for (uint64_t s = 0; s < u; ++s)
        for (uint32_t t = 0; t < a.cntU[s]; ++t)
            if (a.distU[s * a.m + t] != b.distU[s * a.m + t]) return "distU (upper slot " + std::to_string(s) + ", slot " + std::to_string(t) + ")";
    if (!same(a.indeg0, b.indeg0, n)) return "indeg0";
    if (!same(a.lock, b.lock, n)) return "lock";
    if (!same(a.node_id, b.node_id, n)) return "node_id";
    if (!same(a.live, b.live, n) || a.h_live != b.h_live || a.live_count != b.live_count) return "live";
    if (a.h_level != b.h_level || a.h_upper_off != b.h_upper_off || a.h_node_id != b.h_node_id) return "host level / upper_off / node_id";
    auto x = a.id_to_node, y = b.id_to_node;
    std::sort(x.begin(), x.end());
    std::sort(y.begin(), y.end());
    if (x != y) return "id_to_node";
    return std::string();
}

struct Stream {
    std::string name;
    int checkpoints = 0;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    hgc::Graph checkpoint(const HnswIndex& ix, const std::string& label, bool report_orphans, uint64_t* orphans = nullptr)
    {
        hgc::Graph g;
        if (!Probe::snapshot(ix, &g)) fail("FAIL " + name + " [" + label + "]: could not copy the graph back");
        hgc::Reach reach;
        const std::string v = hgc::check(g, &reach, report_orphans);
        if (!v.empty()) fail("FAIL " + name + " [" + label + ", n = " + std::to_string(g.n) + "]: " + v);
        if (orphans) *orphans = reach.orphans;
        ++checkpoints;
        return g;
    }
};

// export `src`, import into a fresh index of the same parameters, compare, then mutate the imported index
void round_trip(Stream& st, const HnswIndex& src, uint32_t dim, bool report_orphans, const std::vector<double>& extra, const std::string& what)
{
    uint64_t src_orphans = 0;
    const hgc::Graph gs = st.checkpoint(src, "source", report_orphans, &src_orphans);
    const uint64_t n = gs.n, nu = gs.n_upper;
    std::vector<uint32_t> cnt0(n), nbr0(n * gs.m0), cntU(nu), nbrU(nu * gs.m);
    std::vector<uint64_t> ids(n);
    std::vector<uint8_t> live(n);
    std::vector<double> rows(n * dim);
    RC(src.graph_export(nullptr, nullptr, cnt0.data(), nbr0.data(), cntU.data(), nbrU.data(), ids.data(), live.data(), rows.data()));
    Owned o;
    o.ix = make(dim, src.metric(), src.params());
    uint64_t orphans = ~0ull;
    RC(o.ix->graph_import(n, ids.data(), live.data(), rows.data(), false, cnt0.data(), nbr0.data(), nu, cntU.data(), nbrU.data(), &orphans));
    double ms[5];
    o.ix->last_import_ms(ms);
    const hgc::Graph gi = st.checkpoint(*o.ix, "imported", report_orphans);
    const std::string d = differs(gs, gi);
    if (!d.empty()) fail("FAIL " + st.name + ": the imported index differs from its source in " + d);
    for (uint64_t i = 0; i < gi.g_cap; ++i)
        if (gi.lock[i] != 0) fail("FAIL " + st.name + ": lock not zero at " + std::to_string(i));
    uint64_t zero_in = 0;
    for (uint64_t i = 0; i < n; ++i) zero_in += gi.indeg0[i] == 0 ? 1 : 0;
    if (n < 2) zero_in = 0;
    if (orphans != zero_in || orphans != src_orphans)
        fail("FAIL " + st.name + ": the import reported " + std::to_string(orphans) + " orphans, " + std::to_string(zero_in) +
             " nodes have no incoming edge, the source's checker counted " + std::to_string(src_orphans));
    if (o.ix->len() != src.len()) fail("FAIL " + st.name + ": len differs");
    {  // a second import into the same handle is refused and changes nothing
        const int rc = o.ix->graph_import(n, ids.data(), live.data(), rows.data(), false, cnt0.data(), nbr0.data(), nu, cntU.data(), nbrU.data(), nullptr);
        if (rc != ERR_INVALID_ARG) fail("FAIL " + st.name + ": an import into a non-empty index returned " + std::to_string(rc));
        const std::string d2 = differs(gi, st.checkpoint(*o.ix, "refused second import", report_orphans));
        if (!d2.empty()) fail("FAIL " + st.name + ": a refused import changed " + d2);
    }
    // the imported index goes on living
    uint64_t at = n;
    {
        const std::vector<uint64_t> nid = ids_of(at, 17);
        RC(o.ix->add_bulk(nid.data(), extra.data(), 17, false));
        at += 17;
        (void)st.checkpoint(*o.ix, "imported + bulk add of 17", report_orphans);
    }
    RC(o.ix->add(id_of(at), extra.data() + (size_t)17 * dim, dim));
    ++at;
    (void)st.checkpoint(*o.ix, "imported + single add", report_orphans);
    uint64_t gone = 0;
    for (uint64_t i = 0; i < n && gone < 2; ++i)  // two nodes that came with the import, then one added since
        if (live[i]) {
            RC(o.ix->remove(ids[i]));
            ++gone;
            (void)st.checkpoint(*o.ix, "imported, delete of node " + std::to_string(i), report_orphans);
        }
    RC(o.ix->remove(id_of(n + 3)));
    const hgc::Graph ge = st.checkpoint(*o.ix, "imported, delete of an added node", report_orphans);
    if (ge.n != n + 18 || o.ix->len() != src.len() + 18 - gone - 1) fail("FAIL " + st.name + ": node or live count wrong after the mutations");
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - st.t0).count();
    printf("stream %s: %d checkpoints %s n=%llu n_upper=%llu orphans=%llu import_ms validate=%.2f ingest=%.2f upload=%.2f keys=%.3f indeg=%.3f %.2f s\n",
           st.name.c_str(), st.checkpoints, what.c_str(), (unsigned long long)n, (unsigned long long)nu, (unsigned long long)orphans, ms[0], ms[1],
           ms[2], ms[3], ms[4], s);
    fflush(stdout);
}

HnswParams params(uint32_t m, uint32_t m0, uint32_t efc, uint64_t seed)
{
    HnswParams p;
    p.m = m;
    p.m0 = m0;
    p.ef_construction = efc;
    p.seed = seed;
    return p;
}

void stream_a()
{
    const struct {
        uint32_t dim;
        int metric;
    } cfg[2] = {{5, EUCLIDEAN}, {100, COSINE}};
    for (const auto& c : cfg) {
        Stream st;
        st.name = "a";
        const uint32_t dim = c.dim;
        const uint64_t n = 2060;
        Owned o;
        o.ix = make(dim, c.metric, params(16, 32, 32, 11));
        std::vector<double> rows = gaussian_rows(0xA000 + dim, n + 18, dim);
        for (uint32_t j = 0; j < dim; ++j) rows[7 * dim + j] = rows[1500 * dim + j] = 0.0;                        // zero rows
        for (uint64_t i = 101; i < 160; ++i) std::memcpy(&rows[i * dim], &rows[100 * dim], dim * sizeof(double));  // 60 copies of one row
        const std::vector<uint64_t> ids = ids_of(0, n);
        RC(o.ix->add_bulk(ids.data(), rows.data(), 1030, false));  // across 1024
        RC(o.ix->add_bulk(ids.data() + 1030, &rows[1030 * dim], n - 1030, false));  // across 2048
        const uint64_t doomed[10] = {0, 1, n - 1, 7, 100, 130, 1023, 1024, 2047, 2048};
        for (uint64_t v : doomed) RC(o.ix->remove(id_of(v)));
        const std::vector<double> extra(rows.begin() + (long)(n * dim), rows.end());
        round_trip(st, *o.ix, dim, false, extra, "dim=" + std::to_string(dim) + " metric=" + std::to_string(c.metric));
    }
}

void stream_b()
{
    const struct {
        uint32_t m, m0;
        int metric;
    } cfg[2] = {{4, 8, MANHATTAN}, {48, 64, DOT}};
    const uint32_t dim = 16;
    const uint64_t n = 600;
    for (const auto& c : cfg) {
        Stream st;
        st.name = "b";
        Owned o;
        o.ix = make(dim, c.metric, params(c.m, c.m0, 32, 23));
        const std::vector<double> rows = gaussian_rows(0xB100 + c.metric, n + 18, dim);
        const std::vector<uint64_t> ids = ids_of(0, n);
        RC(o.ix->add_bulk(ids.data(), rows.data(), 250, false));
        RC(o.ix->add_bulk(ids.data() + 250, &rows[250 * dim], n - 250, false));
        const std::vector<double> extra(rows.begin() + (long)(n * dim), rows.end());
        // lists of 8 cannot promise every node an incoming edge: counted there, refused at m0 = 64
        round_trip(st, *o.ix, dim, c.m0 == 8, extra, "m=" + std::to_string(c.m) + " m0=" + std::to_string(c.m0) + " metric=" + std::to_string(c.metric));
    }
}

void stream_c()
{
    Stream st;
    st.name = "c";
    const uint32_t dim = 3072;
    const uint64_t n = 300;
    Owned o;
    o.ix = make(dim, COSINE, params(16, 32, 32, 31));
    const std::vector<double> rows = gaussian_rows(0xC300, n + 18, dim);
    const std::vector<uint64_t> ids = ids_of(0, n);
    RC(o.ix->add_bulk(ids.data(), rows.data(), n, false));
    const std::vector<double> extra(rows.begin() + (long)(n * dim), rows.end());
    round_trip(st, *o.ix, dim, false, extra, "dim=3072 metric=0");
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string which = argc > 1 ? argv[1] : "";
    if (which == "a") stream_a();
    else if (which == "b") stream_b();
    else if (which == "c") stream_c();
    else {
        printf("usage: hnsw_graph_import_audit a|b|c\n");
        return 2;
    }
    printf("audit ok\n");
    return 0;
}
