// delete_plan.hpp -- the launch plan of a bulk delete (GpuFlatIndex::remove_bulk): which destination rows each launch of the
// row-move kernel (k_move_rows) writes, and whether it may write them in place.  Pure host arithmetic (no HIP):
// tests/native/delete_plan_test.cpp checks its invariants on the CPU and executes every plan against std::remove_if;
// flat_index.cpp runs what this returns once per device array.
//
// n rows, m of them removed at the ascending positions r_0 < ... < r_{m-1}.  The kept row at source position s goes to
// d = s - #{r_i < s}; read from the destination's side, row d comes from s = d + shift(d) with
// shift(d) = #{i : r_i - i <= d} (the keys r_i - i never decrease, so this is one upper_bound).  Rows before r_0 stay.
// The destinations [r_0, n - m) are cut into ascending segments that run in stream order.  One launch moves one segment
// [a, b), its workgroups in no particular order, so it may write in place only if no destination of the launch is a source
// of the launch: b <= a + shift(a), the first source.  Otherwise the segment is gathered into the bounce buffer and copied
// down from there, and must fit it.  One rule gives both: a segment is max(shift(a), rows the bounce holds) long (clipped
// at n - m) and direct iff it is no longer than shift(a).  Few holes: the bounce, in as few chunks as the single delete
// uses.  Once more rows are gone than the bounce holds, the rest of the array moves with one read and one write.  Segments
// need nothing between them but stream order: what [a, b) writes lies below a + shift(a), what any later segment reads lies
// at or above b + shift(b) > b.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace vl {

struct DeleteSegment {
    uint64_t dst_begin, dst_end;  // destination rows [a, b)
    uint64_t shift_begin;         // shift(a): the segment's first source row is a + shift(a)
    uint64_t shift_end;           // shift(b - 1): its last source row is b - 1 + shift(b - 1)
    bool direct;                  // written in place; false: through the bounce buffer
};

// keys[i] = r_i - i for the ascending removed positions: what shift() searches (the kernel reads the same table as u32:
// the caller has checked that the index holds fewer than 2^32 rows)
inline std::vector<uint32_t> delete_keys(const std::vector<uint64_t>& removed)
{
    std::vector<uint32_t> keys(removed.size());
    for (size_t i = 0; i < removed.size(); ++i) keys[i] = (uint32_t)(removed[i] - i);
    return keys;
}

inline uint64_t delete_shift(const std::vector<uint32_t>& keys, uint64_t d)
{
    return (uint64_t)(std::upper_bound(keys.begin(), keys.end(), d, [](uint64_t v, uint32_t k) { return v < (uint64_t)k; }) -
                      keys.begin());
}

// the segments of one array whose bounce buffer holds bounce_rows rows (at least 1)
inline std::vector<DeleteSegment> delete_plan(uint64_t n, const std::vector<uint32_t>& keys, uint64_t bounce_rows)
{
    std::vector<DeleteSegment> plan;
    const uint64_t m = keys.size();
    if (m == 0 || m >= n) return plan;
    bounce_rows = std::max<uint64_t>(bounce_rows, 1);
    const uint64_t end = n - m;
    for (uint64_t a = keys[0]; a < end;) {
        const uint64_t sa = delete_shift(keys, a);
        const uint64_t b = std::min(end, a + std::max(sa, bounce_rows));
        plan.push_back(DeleteSegment{a, b, sa, delete_shift(keys, b - 1), b - a <= sa});
        a = b;
    }
    return plan;
}

}  // namespace vl
