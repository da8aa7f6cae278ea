// hnsw_import_plan.hpp -- structural validation of a caller's HNSW lists before an import touches the device
// (HnswIndex::graph_import, DESIGN.md "Importing a graph").  Plain C++17 on the caller's host arrays: no HIP, no product
// state, so the pass runs under ASan + UBSan in a stand-alone program (tests/native/hnsw_import_plan_test.cpp).
//
// It restates G3 and G4 of the graph audit (tests/native/hnsw_graph_check.hpp) with the audit's labels and wording:
//   G3  cnt0 <= m0, cntU <= m; a listed neighbour is < n, is not the list's owner, and has level >= the list's layer
//   G4  no list names a node twice
// and refuses list capacities outside 1 .. 64 (a wave holds one list; the walk launchers refuse more).
// A G3 violation anywhere is named before a G4 one, as the audit does.  Everything the import kernels index through --
// counts, neighbour ids, levels and upper slots -- is checked here before they run: level[v] is read only after v < n
// held, entries are read only after their count held, and the upper slot of (i, layer) is upper_off[i] + layer - 1 with
// layer <= level[i], which is below n_upper when upper_off[] is the prefix sum of level[] (the caller derives both).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace vl {

constexpr uint32_t HNSW_IMPORT_MAX_LIST = 64;

namespace import_plan_detail {
inline std::string at(const char* inv, const std::string& what, uint64_t node, int layer, int64_t slot)
{
    std::string s = std::string(inv) + ": " + what + " (node " + std::to_string(node) + ", layer " + std::to_string(layer);
    if (slot >= 0) s += ", slot " + std::to_string(slot);
    return s + ")";
}
}  // namespace import_plan_detail

// level[n], upper_off[n]: derived by the caller from the level law, never taken from a file.  cnt0[n], nbr0[n, m0],
// cntU[n_upper], nbrU[n_upper, m] with n_upper = upper_off[n - 1] + level[n - 1].  Returns the first violation or "".
inline std::string hnsw_import_check(uint64_t n, uint32_t m, uint32_t m0, const uint8_t* level, const uint32_t* upper_off,
                                     const uint32_t* cnt0, const uint32_t* nbr0, const uint32_t* cntU, const uint32_t* nbrU)
{
    using import_plan_detail::at;
    if (m == 0 || m > HNSW_IMPORT_MAX_LIST || m0 == 0 || m0 > HNSW_IMPORT_MAX_LIST)
        return "G3: list capacities m = " + std::to_string(m) + ", m0 = " + std::to_string(m0) + " outside 1 .. " +
               std::to_string(HNSW_IMPORT_MAX_LIST);
    if (n == 0) return std::string();
    if (n >= 0xFFFFFFFFull) return "G3: " + std::to_string(n) + " nodes do not fit a 32-bit node index";
    if (!level || !upper_off || !cnt0 || !nbr0) return "G3: a layer-0 array is missing";
    std::vector<uint32_t> stamp(n, 0xFFFFFFFFu);  // stamp[v] = serial of the last list that named v
    uint32_t serial = 0;
    for (int pass = 3; pass <= 4; ++pass) {
        for (uint64_t i = 0; i < n; ++i) {
            for (int layer = 0; layer <= (int)level[i]; ++layer) {
                const uint32_t cap = layer == 0 ? m0 : m;
                const uint64_t slot = layer == 0 ? i : (uint64_t)upper_off[i] + (uint64_t)(layer - 1);
                if (layer > 0 && (!cntU || !nbrU)) return "G3: an upper-layer array is missing";
                const uint32_t cnt = layer == 0 ? cnt0[i] : cntU[slot];
                if (cnt > cap) return at("G3", "count " + std::to_string(cnt) + " > capacity " + std::to_string(cap), i, layer, -1);
                const uint32_t* nb = layer == 0 ? nbr0 + i * m0 : nbrU + slot * m;
                if (pass == 4) ++serial;  // at most n + n_upper < 2^32 - 1 lists
                for (uint32_t t = 0; t < cnt; ++t) {
                    const uint32_t v = nb[t];
                    if (pass == 3) {
                        if (v >= n) return at("G3", "neighbour " + std::to_string(v) + " >= n", i, layer, t);
                        if (v == i) return at("G3", "a node lists itself", i, layer, t);
                        if ((int)level[v] < layer)
                            return at("G3", "neighbour " + std::to_string(v) + " of level " + std::to_string(level[v]) + " listed above its level", i, layer, t);
                    } else {
                        if (stamp[v] == serial) return at("G4", "neighbour " + std::to_string(v) + " named twice", i, layer, t);
                        stamp[v] = serial;
                    }
                }
            }
        }
    }
    return std::string();
}

}  // namespace vl
