// update_plan.hpp -- the host plan of an in-place update / upsert (GpuFlatIndex::update_bulk): which storage position each
// listed row overwrites, which rows are appended, and how the overwritten positions are cut into staging chunks.  Pure host
// arithmetic (no HIP): tests/native/update_plan_test.cpp executes every plan against the sequential loop on the CPU.
//
// The call's contract is the loop `for i < n: contains(ids[i]) ? update(ids[i], values_i) : (insert_missing ? add(ids[i],
// values_i) : fail)`, where update() rewrites the FIRST row carrying the id (get_vector's rule).  Read from the end of the
// loop: every distinct listed id that the table holds names one position -- the first one carrying it -- and that row ends
// with the values of the id's LAST occurrence in the list; every distinct absent id is appended once, in the order of the
// absent ids' first occurrences (the first occurrence adds the row, the later ones find it and update it), and holds the
// values of its last occurrence too.  A missing id without insert_missing refuses the whole call: the first such id in
// list order is reported and nothing is planned.
//
// Lookup: the distinct listed ids go into an open-addressing table (a power of two of slots, at most half full, linear
// probing) behind a bitmap of the same hash's top bits, as remove_bulk's does; one forward walk over the position -> id
// table fills in each id's first position and stops once every listed id has one.  No scan per id.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace vl {

struct UpdatePlan {
    bool refused = false;     // an id is absent and insert_missing is off: nothing below is filled in
    uint64_t missing_id = 0;  // the first such id in list order
    // rows rewritten in place: position pos[j] takes the values of list entry src[j]; pos strictly ascending
    std::vector<uint64_t> pos, src;
    // rows appended, in order: id append_ids[j] with the values of list entry append_src[j]
    std::vector<uint64_t> append_ids, append_src;
};

inline UpdatePlan update_plan(const uint64_t* row_ids, uint64_t rows, const uint64_t* ids, uint64_t n, bool insert_missing)
{
    UpdatePlan plan;
    if (n == 0) return plan;
    constexpr uint64_t NONE = ~0ull;
    struct Slot {
        uint64_t id;
        uint64_t first_pos;  // NONE: not (yet) seen in the table
        uint64_t last_src;   // the id's last occurrence in the list
        uint64_t first_src;  // ... and its first (orders the appended rows, names the refusal)
        bool used;
    };
    int log2_slots = 4, log2_bits = 10;
    while ((1ull << log2_slots) < 2 * n) ++log2_slots;
    while (log2_bits < 30 && (1ull << log2_bits) < 8 * n) ++log2_bits;
    std::vector<Slot> table((size_t)1 << log2_slots, Slot{0, NONE, 0, 0, false});
    std::vector<uint64_t> maybe((size_t)1 << (log2_bits - 6), 0);
    const uint64_t mask = table.size() - 1;
    const auto hash = [](uint64_t id) { return id * 0x9E3779B97F4A7C15ull; };
    uint64_t distinct = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t h = hash(ids[i]), b = h >> (64 - log2_bits);
        maybe[b >> 6] |= 1ull << (b & 63);
        uint64_t s = h >> (64 - log2_slots);
        while (table[s].used && table[s].id != ids[i]) s = (s + 1) & mask;
        if (!table[s].used) {
            table[s] = Slot{ids[i], NONE, i, i, true};
            ++distinct;
        } else {
            table[s].last_src = i;
        }
    }
    uint64_t found = 0;
    for (uint64_t p = 0; p < rows && found < distinct; ++p) {
        const uint64_t id = row_ids[p], h = hash(id), b = h >> (64 - log2_bits);
        if (!((maybe[b >> 6] >> (b & 63)) & 1)) continue;
        uint64_t s = h >> (64 - log2_slots);
        while (table[s].used && table[s].id != id) s = (s + 1) & mask;
        if (table[s].used && table[s].first_pos == NONE) {
            table[s].first_pos = p;
            ++found;
        }
    }
    std::vector<std::pair<uint64_t, uint64_t>> hits, adds;  // (position, source), (first occurrence, slot)
    hits.reserve(found);
    uint64_t first_missing = NONE;
    for (size_t s = 0; s < table.size(); ++s) {
        const Slot& t = table[s];
        if (!t.used) continue;
        if (t.first_pos != NONE) {
            hits.emplace_back(t.first_pos, t.last_src);
        } else {
            adds.emplace_back(t.first_src, (uint64_t)s);
            first_missing = std::min(first_missing, t.first_src);
        }
    }
    if (!adds.empty() && !insert_missing) {
        plan.refused = true;
        plan.missing_id = ids[first_missing];
        return plan;
    }
    std::sort(hits.begin(), hits.end());
    std::sort(adds.begin(), adds.end());
    plan.pos.reserve(hits.size());
    plan.src.reserve(hits.size());
    for (const auto& h : hits) {
        plan.pos.push_back(h.first);
        plan.src.push_back(h.second);
    }
    plan.append_ids.reserve(adds.size());
    plan.append_src.reserve(adds.size());
    for (const auto& a : adds) {
        plan.append_ids.push_back(table[a.second].id);
        plan.append_src.push_back(table[a.second].last_src);
    }
    return plan;
}

// rows of `dim` f64 values one staging buffer of stage_bytes holds: per row its values, its position (u32) and its new flag
// (a byte), the two side arrays each rounded up to 16 bytes.  At least 1 (the caller allocates update_stage_bytes(1) then).
inline uint64_t update_stage_rows(uint64_t stage_bytes, uint64_t dim)
{
    const uint64_t per_row = dim * 8 + 5;
    return stage_bytes > 48 + per_row ? (stage_bytes - 48) / per_row : 1;
}
// byte offsets of the positions and of the flags within a staging buffer laid out for `rows` rows, and its size
inline uint64_t update_stage_pos_offset(uint64_t rows, uint64_t dim) { return (rows * dim * 8 + 15) / 16 * 16; }
inline uint64_t update_stage_flag_offset(uint64_t rows, uint64_t dim) { return update_stage_pos_offset(rows, dim) + (rows * 4 + 15) / 16 * 16; }
inline uint64_t update_stage_bytes(uint64_t rows, uint64_t dim) { return update_stage_flag_offset(rows, dim) + (rows + 15) / 16 * 16; }

// the cut of the m planned positions into chunks [begin, end) of at most stage_rows rows, in ascending position order
inline std::vector<std::pair<uint64_t, uint64_t>> update_chunks(uint64_t m, uint64_t stage_rows)
{
    std::vector<std::pair<uint64_t, uint64_t>> cuts;
    stage_rows = std::max<uint64_t>(stage_rows, 1);
    for (uint64_t a = 0; a < m; a += stage_rows) cuts.emplace_back(a, std::min(m, a + stage_rows));
    return cuts;
}

}  // namespace vl
