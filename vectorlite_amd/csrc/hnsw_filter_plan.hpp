// hnsw_filter_plan.hpp -- how one id-filtered HNSW search is answered (HnswIndex::search_filtered).
// Plain C++17 on five numbers: no HIP, no product state, so it runs under ASan + UBSan in a stand-alone program
// (tests/native/hnsw_filter_plan_test.cpp).
//
//   n_pass          passing nodes now (live and in the filter's id set)
//   max_candidates  = min(k, n_pass)
//   ef_walk         = ef ? max(max_candidates, ef) : max(max_candidates, min_beam)
//   EXACT route     n_pass == 0 (zero results), or ef_walk > 512, or ef_walk * n_nodes > 256 * n_pass -- the window a
//                   walk would need to hold ef_walk passing entries is expected to exceed half the largest list
//   WALK route      otherwise, with cap = the smallest of 64 / 128 / 256 / 512 that is
//                   >= max(ef_walk, ceil(2 * ef_walk * n_nodes / n_pass)); 512 if none is
// 256 and the factor 2 are capacity arguments, not measured optima.  Every product is formed in 128 bits.
#pragma once

#include <cstdint>

namespace vl {

constexpr uint64_t HNSW_FILTER_MAX_LIST = 512;    // the walk's largest list (HNSW_MAX_EF)
constexpr uint64_t HNSW_FILTER_EXACT_RATIO = 256; // exact route when ef_walk * n_nodes > this * n_pass

struct HnswFilterPlan {
    int route = 1;  // 0 walk, 1 exact
    uint32_t cap = 0;  // walk route only
    uint64_t max_candidates = 0;
    uint64_t ef_walk = 0;
};

inline HnswFilterPlan hnsw_filter_plan(uint64_t k, uint32_t ef, uint32_t min_beam, uint64_t n_nodes, uint64_t n_pass)
{
    typedef unsigned __int128 u128;
    HnswFilterPlan p;
    p.max_candidates = k < n_pass ? k : n_pass;
    const uint64_t floor = ef ? (uint64_t)ef : (uint64_t)min_beam;
    p.ef_walk = p.max_candidates > floor ? p.max_candidates : floor;
    if (n_pass == 0 || p.ef_walk == 0 || p.ef_walk > HNSW_FILTER_MAX_LIST) return p;  // ef_walk == 0: k == 0, nothing to return
    if ((u128)p.ef_walk * n_nodes > (u128)HNSW_FILTER_EXACT_RATIO * n_pass) return p;
    // ceil(2 ef n / n_pass) <= 512 here: 2 ef n <= 512 n_pass
    const u128 twice = (u128)2 * p.ef_walk * n_nodes;
    uint64_t need = (uint64_t)((twice + n_pass - 1) / n_pass);
    if (need < p.ef_walk) need = p.ef_walk;
    p.route = 0;
    p.cap = need <= 64 ? 64u : (need <= 128 ? 128u : (need <= 256 ? 256u : 512u));
    return p;
}

}  // namespace vl
