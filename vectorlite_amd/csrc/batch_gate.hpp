// batch_gate.hpp -- may this call use the bf16 MFMA filter?  One struct of the facts a route reads and one pure function per
// route.  No HIP: GpuFlatIndex::batch_gate() fills the struct -- the only reader of VL_MFMA and
// VL_MFMA_MIN_BATCH -- and tests/native/batch_gate_test.cpp checks every function on the CPU.
#pragma once

#include <stdint.h>

#include "examples_plan.hpp"
#include "masked_batch_plan.hpp"

namespace vl {

struct BatchGate {
    int forced_path;          // force_path(): 0 = none
    uint64_t out_of_domain;   // rows outside the fast-path domain
    uint64_t dim;
    uint64_t rows;            // len()
    uint64_t nq;
    uint64_t k_eff;
    bool env_off;             // VL_MFMA starts with '0'
    bool scan_supported;      // mfma_scan_supported(dim, metric)
    bool rows_kernel;         // mfma_rows_kernel(dim): the row-stationary kernel, the only one with a masked and a range form
    MaskedBatchLimits lim;    // min_batch: VL_MFMA_MIN_BATCH, else MFMA_MIN_BATCH
};

// what every route but the join asks: nothing forced, no row whose key could be NaN, the filter not switched off, a kernel
// shape for (dim, metric)
inline bool gate_core(const BatchGate& g)
{
    return g.forced_path == 0 && g.out_of_domain == 0 && !g.env_off && g.scan_supported;
}

// search_batch on host or device queries: the list's margin, the minimum batch, and the row floor of the sampling pass
inline bool gate_topk(const BatchGate& g)
{
    return gate_core(g) && g.nq > 1 && g.k_eff <= g.lim.k_max && g.nq >= g.lim.min_batch && g.rows >= g.lim.min_rows;
}

// The deep-k batch: gate_topk with k_eff above the list's margin, up to `deep_max_k`
// (VL_DEEP_MAX_K), on the row-stationary kernel.  Never true together with gate_topk.
inline bool gate_deep(const BatchGate& g, uint64_t deep_max_k = 1024)
{
    return gate_core(g) && g.rows_kernel && g.nq > 1 && g.k_eff > g.lim.k_max && g.k_eff <= deep_max_k && g.nq >= g.lim.min_batch &&
           g.rows >= g.lim.min_rows;
}

// ... written into a shard's exchange record at stride ks: the record's planes are indexed with 32-bit words
inline bool gate_record(const BatchGate& g, uint64_t ks)
{
    return gate_topk(g) && g.nq * ks < (1ull << 31);
}

// The index_ok of the *_batch_plan.hpp shapes (they add min_rows, min_batch and k_max per query).  mfma_scan_supported holds
// for dim 0 (its rows pad to 128 like any dim <= 128), so the zero-length row is a term of its own: these entry points
// accept a null query pointer there, which the pass's staging must not be handed.
inline bool gate_tail_index(const BatchGate& g)
{
    return gate_core(g) && g.dim != 0;
}

// ... of the masked batch, which always runs under a bitmap (the grouped and MMR batches need one only with a filter and
// ask rows_kernel through their plan)
inline bool gate_masked_index(const BatchGate& g)
{
    return gate_tail_index(g) && g.rows_kernel;
}

// The batched range search; g.nq = the queries in front of the first NaN threshold.  No row floor: the top-k batch's floor
// belongs to its sampling pass, and this route has none.
inline bool gate_range(const BatchGate& g, bool filtered)
{
    return !filtered && g.nq >= g.lim.min_batch && gate_core(g) && g.rows_kernel;
}

// The self-join: its own kernel, so join_rows_supported(dim, metric) in mfma_scan_supported's place; `cosine` = the metric
// has a pass on the call's route (cosine always; Euclidean and dot when the route is mfma); positions travel as 31-bit
// halves of a pair; one call is one pass, so no minimum batch.
inline bool gate_join(const BatchGate& g, bool route_loop, bool cosine, bool join_rows_supported)
{
    return !route_loop && cosine && g.forced_path == 0 && g.out_of_domain == 0 && !g.env_off && join_rows_supported &&
           g.rows < 0x7FFFFFFFull;
}

// The nearest-label assignment: g.nq = the labels.  `route_exact` = the caller asked for the exact
// route; `has_pass` = cosine, Euclidean or dot; `labels_in_domain` = every label is inside the fast-path domain.  Row
// positions travel as 32-bit words in whole 32-row blocks.  No row floor: there is no sampling pass.
inline bool gate_assign(const BatchGate& g, bool route_exact, bool has_pass, bool labels_in_domain)
{
    return !route_exact && has_pass && g.rows_kernel && gate_tail_index(g) && labels_in_domain && g.rows < 0xFFFFFFE0ull;
}

// The k-nearest-neighbour graph: g.k_eff = k, g.nq unused.  gate_assign's conditions without labels;
// on top of them every row must have k other rows (len - 1 >= k), or each row keeps every other row and the exact route
// answers.
inline bool gate_knn(const BatchGate& g, bool route_exact, bool has_pass)
{
    return !route_exact && has_pass && g.rows_kernel && gate_tail_index(g) && g.rows < 0xFFFFFFE0ull && g.rows >= 1 &&
           g.rows - 1 >= g.k_eff;
}

// The search by examples: g.nq = the examples, g.k_eff = k.  gate_assign's conditions with the forced
// path in the route setter's place (gate_core reads it); on top of them the seed list must hold k rows.  `has_pass` =
// cosine, Euclidean or dot; `examples_in_domain` = every positive and negative is inside the fast-path domain.
inline bool gate_examples(const BatchGate& g, bool has_pass, bool examples_in_domain)
{
    return has_pass && g.rows_kernel && gate_tail_index(g) && examples_in_domain && g.rows < 0xFFFFFFE0ull &&
           g.k_eff <= EXAMPLES_FAST_MAX_K;
}

}  // namespace vl
