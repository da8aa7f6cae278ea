// vectorlite_amd/csrc/hnsw_import_plan.hpp on the CPU (stand-alone, run under ASan + UBSan by
// tests/test_hnsw_import_plan_cpu.py): the structural pass an HNSW graph import makes before any device work.
// Every array is a std::vector of exactly the size the contract names, so a read past a count, a node or a slot is an
// ASan report.  Hand-made graphs, each expectation the exact message:
//   - n = 0 (null arrays), n = 1 with an empty list;
//   - a list exactly at capacity for m0 = 32 and m0 = 64, and one entry over it; capacities outside 1 .. 64;
//   - a graph with two nodes of level 15 naming each other on every layer;
//   - each G3 and G4 violation alone, in layer 0 and in an upper layer, at slot 0 and at the last slot (a node named
//     twice is reported at the LATER of the two slots, so the pairs are (0, 1) and (0, last));
//   - a G3 violation in a later node is named before a G4 violation in an earlier one, as the graph audit does.
#include "../../vectorlite_amd/csrc/hnsw_import_plan.hpp"

#include <cstdio>
#include <string>
#include <vector>

namespace {
int failures = 0;

struct G {
    uint64_t n = 0;
    uint32_t m = 0, m0 = 0;
    std::vector<uint8_t> level;
    std::vector<uint32_t> upper_off, cnt0, nbr0, cntU, nbrU;

    G(uint32_t m_, uint32_t m0_, const std::vector<uint8_t>& levels) : n(levels.size()), m(m_), m0(m0_), level(levels)
    {
        uint32_t run = 0;
        for (uint8_t l : level) {
            upper_off.push_back(run);
            run += l;
        }
        cnt0.assign(n, 0);
        nbr0.assign(n * m0, 0xDEADBEEFu);  // unused slots hold a value that would fail every check if it were read
        cntU.assign(run, 0);
        nbrU.assign((size_t)run * m, 0xDEADBEEFu);
    }
    void set0(uint32_t i, const std::vector<uint32_t>& l)
    {
        cnt0[i] = (uint32_t)l.size();
        for (size_t t = 0; t < l.size() && t < m0; ++t) nbr0[(size_t)i * m0 + t] = l[t];
    }
    void setU(uint32_t i, int layer, const std::vector<uint32_t>& l)
    {
        const uint32_t s = upper_off[i] + (uint32_t)(layer - 1);
        cntU[s] = (uint32_t)l.size();
        for (size_t t = 0; t < l.size() && t < m; ++t) nbrU[(size_t)s * m + t] = l[t];
    }
    std::string check() const
    {
        return vl::hnsw_import_check(n, m, m0, level.data(), upper_off.data(), cnt0.data(), nbr0.data(), cntU.data(), nbrU.data());
    }
};

void expect(const char* what, const std::string& got, const std::string& want)
{
    if (got != want) {
        printf("FAIL %s:\n  got  \"%s\"\n  want \"%s\"\n", what, got.c_str(), want.c_str());
        ++failures;
    }
}

// six nodes, m = 3, m0 = 4; nodes 0, 2, 4, 5 on level 1 (slots 0, 1, 2, 3); every list full
G base()
{
    G g(3, 4, {1, 0, 1, 0, 1, 1});
    for (uint32_t i = 0; i < 6; ++i) g.set0(i, {(i + 1) % 6, (i + 2) % 6, (i + 3) % 6, (i + 4) % 6});
    g.setU(0, 1, {2, 4, 5});
    g.setU(2, 1, {0, 4, 5});
    g.setU(4, 1, {0, 2, 5});
    g.setU(5, 1, {0, 2, 4});
    return g;
}
}  // namespace

int main()
{
    expect("n = 0", vl::hnsw_import_check(0, 16, 32, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "");
    {
        G g(16, 32, {0});
        expect("n = 1, empty list", g.check(), "");
        g.set0(0, {0});
        expect("n = 1 listing itself", g.check(), "G3: a node lists itself (node 0, layer 0, slot 0)");
    }
    expect("m = 65", vl::hnsw_import_check(0, 65, 32, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
           "G3: list capacities m = 65, m0 = 32 outside 1 .. 64");
    expect("m0 = 0", vl::hnsw_import_check(0, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
           "G3: list capacities m = 16, m0 = 0 outside 1 .. 64");
    expect("m0 = 65", G(16, 65, {0, 0}).check(), "G3: list capacities m = 16, m0 = 65 outside 1 .. 64");

    for (uint32_t m0 : {32u, 64u}) {  // a list exactly at capacity, then one over (the extra entry does not exist)
        G g(16, m0, std::vector<uint8_t>(m0 + 2, 0));
        std::vector<uint32_t> l;
        for (uint32_t v = 1; v <= m0; ++v) l.push_back(v);
        g.set0(0, l);
        g.set0(m0 + 1, l);  // the last node: its list ends with the array
        expect("list at capacity", g.check(), "");
        g.cnt0[m0 + 1] = m0 + 1;
        expect("list over capacity", g.check(),
               "G3: count " + std::to_string(m0 + 1) + " > capacity " + std::to_string(m0) + " (node " + std::to_string(m0 + 1) + ", layer 0)");
        g.cnt0[m0 + 1] = m0;
        g.nbr0[(size_t)(m0 + 1) * m0 + m0 - 1] = 1;  // the last slot of the last list repeats its first
        expect("duplicate at the last slot of a full list", g.check(),
               "G4: neighbour 1 named twice (node " + std::to_string(m0 + 1) + ", layer 0, slot " + std::to_string(m0 - 1) + ")");
    }

    {  // level 15: nodes 0 and 2 name each other on layers 1 .. 15 (30 upper slots)
        G g(2, 4, {15, 0, 15});
        g.set0(0, {1, 2});
        g.set0(1, {0});
        g.set0(2, {1});
        for (int layer = 1; layer <= 15; ++layer) {
            g.setU(0, layer, {2});
            g.setU(2, layer, {0});
        }
        expect("level 15", g.check(), "");
        g.setU(2, 15, {1});
        expect("level 15, a level-0 node on layer 15", g.check(), "G3: neighbour 1 of level 0 listed above its level (node 2, layer 15, slot 0)");
        g.setU(2, 15, {0, 0});
        expect("level 15, duplicate on layer 15", g.check(), "G4: neighbour 0 named twice (node 2, layer 15, slot 1)");
        g.setU(2, 15, {0, 1, 1});
        expect("level 15, count over m on the last slot", g.check(), "G3: count 3 > capacity 2 (node 2, layer 15)");
    }

    expect("base graph", base().check(), "");
    // layer 0: the list of node 1 (level 0), slots 0 and 3; layer 1: the list of node 5 (the last upper slot), slots 0 and 2
    for (int upper = 0; upper <= 1; ++upper) {
        const uint32_t owner = upper ? 5 : 1, last = upper ? 2 : 3;
        const int layer = upper;
        const std::string where_owner = "(node " + std::to_string(owner) + ", layer " + std::to_string(layer);
        auto entry = [&](G& g, uint32_t slot) -> uint32_t& {
            return upper ? g.nbrU[(size_t)(g.upper_off[owner]) * g.m + slot] : g.nbr0[(size_t)owner * g.m0 + slot];
        };
        for (uint32_t slot : {0u, last}) {
            const std::string where = where_owner + ", slot " + std::to_string(slot) + ")";
            {
                G g = base();
                entry(g, slot) = 6;
                expect("neighbour = n", g.check(), "G3: neighbour 6 >= n " + where);
                entry(g, slot) = 0xFFFFFFFFu;
                expect("neighbour = NONE", g.check(), "G3: neighbour 4294967295 >= n " + where);
            }
            {
                G g = base();
                entry(g, slot) = owner;
                expect("self loop", g.check(), "G3: a node lists itself " + where);
            }
            if (upper) {
                G g = base();
                entry(g, slot) = 3;
                expect("above its level", g.check(), "G3: neighbour 3 of level 0 listed above its level " + where);
            }
        }
        {
            G g = base();
            (upper ? g.cntU[g.upper_off[owner]] : g.cnt0[owner]) = last + 2;
            expect("count over capacity", g.check(),
                   "G3: count " + std::to_string(last + 2) + " > capacity " + std::to_string(last + 1) + " " + where_owner + ")");
        }
        for (uint32_t later : {1u, last}) {  // slot 0 named again at slot 1, and at the last slot
            G g = base();
            const uint32_t v = entry(g, 0);
            entry(g, later) = v;
            expect("named twice", g.check(),
                   "G4: neighbour " + std::to_string(v) + " named twice " + where_owner + ", slot " + std::to_string(later) + ")");
        }
    }
    {  // a shorter count hides what lies behind it: entries at and past the count are never read
        G g = base();
        g.cnt0[1] = 2;
        g.nbr0[1 * 4 + 2] = 77;
        g.nbr0[1 * 4 + 3] = 1;
        expect("entries past the count", g.check(), "");
    }
    {  // G3 anywhere before G4 anywhere
        G g = base();
        g.nbr0[0 * 4 + 1] = g.nbr0[0 * 4 + 0];  // G4 in node 0
        g.nbrU[(size_t)3 * 3 + 2] = 9;          // G3 in node 5, layer 1
        expect("G3 before G4", g.check(), "G3: neighbour 9 >= n (node 5, layer 1, slot 2)");
    }

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("hnsw import plan ok\n");
    return 0;
}
