// join.hip -- the similarity self-join's candidate pass: a triangular bf16 MFMA pass in which both
// operands are blocks of the index's own fragment-major slab.
//
// k_join_rows<KSTEPS, METRIC> is a symmetric rank-k update on the matrix cores (v_mfma_f32_16x16x32_bf16):
//   B = a column PANEL of QPB consecutive stored rows (128; 96 at stride 768), copied once per stretch into LDS as it lies
//       in the slab.  For the 16x16x32 shape lane (c16, kg) of a B fragment holds column c16, k-group kg -- the piece order
//       of an A fragment -- so a 1 KB slab chunk IS a B fragment: no re-layout, no row padding, one ds_read_b128 per lane
//       at lane * 16 (consecutive lanes, consecutive 16 bytes: conflict-free), and QPB x row bytes is the whole panel.
//   A = 32-row blocks at or below the panel, streamed by the waves: one contiguous 1 KB load per fragment, held for a K
//       phase (the whole K up to stride 384, four phases at 512 and 768) and refilled right behind its last use with the
//       wave's next block, so a load has a whole block's MFMAs to land.
//   C = a 32 x QPB tile per wave: every A fragment feeds QPB / 16 MFMAs, every B fragment two.
// join_plan.hpp deals the (panel, block) units to the workgroups.  One scalar threshold serves the whole launch: the
// epilogue is a max tree over the tile (cosine: over the sums; Euclidean and dot: over join_pair_key of each sum and the
// two rows' norms), one compare and one branch; the candidate code behind it keeps pos_a < pos_b <
// n_rows (which drops the mirrored half of a diagonal unit, the self pair and the rows past the end) and appends
// (pos_a, pos_b, key) to the wave's LDS ring; a flush reserves its entries in the global buffer with ONE returning atomic.
#include "join.hpp"

#include <type_traits>

#include "device_common.hpp"
#include "mfma_scan.hpp"

namespace vl {

static_assert(JOIN_IN_EXTRA == IN_EXTRA_MFMA, "the join's keys are the batch filter's keys");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int JOIN_NW = 8;     // waves per workgroup (two per SIMD)
constexpr int JOIN_SEG = 128;  // ring entries per wave: a flush whenever the next 64 might not fit, so it never overflows

__device__ __forceinline__ float jmax3(float a, float b, float c)
{
    return __builtin_fmaxf(__builtin_fmaxf(a, b), c);  // folds to v_max3_f32
}

// METRIC: COSINE compares the key itself.  DOT and EUCLIDEAN compare join_pair_key (join_plan.hpp) of the key and the row's
// and the column's f32 norms: row_norm is norm16, e32 is join_pair_e32.
template <int KSTEPS, int METRIC>
__global__ __launch_bounds__(JOIN_NW * 64) void k_join_rows(const unsigned char* __restrict__ slab, uint32_t n_rows, uint32_t y0,
                                                            uint32_t y1, float thr, JoinCand* __restrict__ cand,
                                                            uint32_t* __restrict__ cnt, uint32_t cap,
                                                            const float* __restrict__ row_norm, float e32)
{
    constexpr int LDB = KSTEPS * 16;
    constexpr int ROW_BYTES = LDB * 2;
    constexpr int KS32 = KSTEPS / 2;                       // K = 32 per MFMA
    constexpr int QPB = (int)join_qpb((uint32_t)LDB);
    constexpr int QB = QPB / 16;                           // column blocks of the panel
    constexpr int PH = KS32 > 12 ? 4 : 1;                  // K phases: 16 = 4 x 4 (stride 512), 24 = 4 x 6 (stride 768)
    constexpr int KSP = KS32 / PH;                         // A fragments a wave holds per 16-row half block
    constexpr int GROUP_BYTES = 16 * ROW_BYTES;            // one 16-row group of the slab: KS32 chunks of 1 KB
    constexpr bool PAIR = METRIC != COSINE;                // per-pair scalars in the epilogue
    constexpr int COL_BYTES = PAIR ? QPB * 4 : 0;          // the panel rows' norms
    static_assert(KS32 % PH == 0 && QPB % 32 == 0, "whole K phases; panels are whole row blocks");
    static_assert(QPB * ROW_BYTES + JOIN_NW * JOIN_SEG * 12 + COL_BYTES <= 160 * 1024, "panel, rings and column scalars fit the LDS");

    __shared__ __attribute__((aligned(16))) unsigned char lds[QPB * ROW_BYTES + JOIN_NW * JOIN_SEG * 12 + COL_BYTES];
    unsigned char* panel = lds;                                                       // [QB][KS32] chunks of 1 KB
    uint32_t* ring_a = reinterpret_cast<uint32_t*>(lds + (size_t)QPB * ROW_BYTES);    // [NW][SEG]
    uint32_t* ring_b = ring_a + JOIN_NW * JOIN_SEG;
    float* ring_key = reinterpret_cast<float*>(ring_b + JOIN_NW * JOIN_SEG);
    float* col_n = ring_key + JOIN_NW * JOIN_SEG;  // [QPB] (PAIR)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, kg = lane >> 4;
    const uint32_t lane_off = (uint32_t)lane * 16u;

    const JoinPlan plan = join_plan(n_rows, (uint32_t)QPB);
    uint64_t u, u_end;
    join_wg_units(plan, y0, y1, join_wg_rank(blockIdx.x, gridDim.x), gridDim.x, &u, &u_end);
    if (u >= u_end) return;  // workgroup-uniform
    uint32_t y = join_unit_panel(plan, u);
    const uint32_t n_groups = (n_rows + 15u) / 16u;  // 16-row groups that hold a row (the slab is allocated beyond them)

    uint32_t my_cnt = 0;
    uint32_t* my_a = ring_a + wave * JOIN_SEG;
    uint32_t* my_b = ring_b + wave * JOIN_SEG;
    float* my_key = ring_key + wave * JOIN_SEG;
    auto flush_wave = [&]() {  // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(cnt, my_cnt);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        for (uint32_t e = lane; e < my_cnt; e += 64) {
            const uint32_t slot = base + e;
            if (slot < cap) {  // a counter above cap tells the host that this launch's range has to be split
                JoinCand c;
                c.a = my_a[e];
                c.b = my_b[e];
                c.key = my_key[e];
                cand[slot] = c;
            }
        }
        my_cnt = 0;
    };

    auto a_ptr = [&](uint32_t blk) { return slab + (size_t)blk * (2 * GROUP_BYTES) + lane_off; };
    bf16x8 afrag[2][KSP];

    for (; u < u_end; ++y) {  // one stretch of one panel per turn: workgroup-uniform
        const uint32_t b0 = (uint32_t)(u - join_units_before(plan, y));
        const uint32_t nb = join_panel_blocks(plan, y);
        const uint32_t b1 = (uint64_t)(nb - b0) <= u_end - u ? nb : b0 + (uint32_t)(u_end - u);
        u += b1 - b0;
        const uint32_t col0 = y * (uint32_t)QPB;

        // this wave's blocks of the stretch: b0 + wave, + NW, ...; the first one's fragments are requested before the panel
        uint32_t b = b0 + (uint32_t)wave;
        const bool has_work = b < b1;
        const uint32_t b_last = has_work ? b + ((b1 - 1 - b) / JOIN_NW) * JOIN_NW : b0;  // a valid block to re-read at the tail
        if (has_work) {
            const unsigned char* p = a_ptr(b);
#pragma unroll
            for (int s = 0; s < KSP; ++s)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) afrag[rb][s] = *reinterpret_cast<const bf16x8*>(p + rb * GROUP_BYTES + s * 1024);
        }

        // ---- the panel -> LDS, as it lies in the slab; groups past the last row are zeros (they are never allocated) ----
        __syncthreads();  // the previous panel is consumed
        {
            constexpr int PIECES = QPB * ROW_BYTES / 16;
            constexpr int GROUP_PIECES = GROUP_BYTES / 16;
            const unsigned char* src = slab + (size_t)col0 * ROW_BYTES;
            const uint32_t g0 = col0 / 16u;
            for (int c = tid; c < PIECES; c += JOIN_NW * 64) {
                u32x4 v = u32x4{0u, 0u, 0u, 0u};
                if (g0 + (uint32_t)(c / GROUP_PIECES) < n_groups) v = *reinterpret_cast<const u32x4*>(src + (size_t)c * 16);
                *reinterpret_cast<u32x4*>(panel + (size_t)c * 16) = v;
            }
            if (PAIR && tid < QPB) {  // the panel rows' norms next to it; rows past the end are zero rows
                const uint32_t pos = col0 + (uint32_t)tid;
                col_n[tid] = pos < n_rows ? row_norm[pos] : 0.f;
            }
        }
        __syncthreads();

        for (; b < b1; b += JOIN_NW) {
            const uint32_t nxt = b + JOIN_NW < b1 ? b + JOIN_NW : b_last;
            const unsigned char* pn = a_ptr(nxt);
            const unsigned char* pc = a_ptr(b);
            const uint32_t row0 = b * JOIN_BLOCK_ROWS;
            // the norms of this lane's rows 16 rb + 4 kg + jj, requested in front of the MFMAs (the array is allocated in whole
            // 64-row tiles; entries past the last row are never part of a kept pair)
            f32x4 ra[2];
            if (PAIR) {
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) ra[rb] = *reinterpret_cast<const f32x4*>(row_norm + row0 + 16 * rb + 4 * kg);
            }
            f32x4 acc[2][QB];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int j = 0; j < QB; ++j) acc[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ph = 0; ph < PH; ++ph) {
                // the fragments are refilled behind their last use: with this block's next K phase, or the next block's first
                const unsigned char* psrc = ph + 1 < PH ? pc + (size_t)(ph + 1) * KSP * 1024 : pn;
#pragma unroll
                for (int s = 0; s < KSP; ++s) {
                    const unsigned char* bp = panel + (size_t)(ph * KSP + s) * 1024 + lane_off;
#pragma unroll
                    for (int j = 0; j < QB; ++j) {
                        const bf16x8 bq = *reinterpret_cast<const bf16x8*>(bp + (size_t)j * GROUP_BYTES);
                        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[0][s], bq, acc[0][j], 0, 0, 0);
                        acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[1][s], bq, acc[1][j], 0, 0, 0);
                    }
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb)
                        afrag[rb][s] = *reinterpret_cast<const bf16x8*>(psrc + rb * GROUP_BYTES + s * 1024);
                }
            }
            // ---- epilogue: C layout of a 16x16 block: column = lane & 15 (panel row), row = 4 (lane >> 4) + reg ----
            auto append = [&](bool is_cand, uint32_t pos_a, uint32_t pos_b, float key) {  // wave-uniform call
                const unsigned long long mk = __builtin_amdgcn_ballot_w64(is_cand);
                if (mk == 0ull) return;
                if (my_cnt + 64u > (uint32_t)JOIN_SEG) flush_wave();
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
                if (is_cand) {
                    const uint32_t e = my_cnt + rank;
                    my_a[e] = pos_a;
                    my_b[e] = pos_b;
                    my_key[e] = key;
                }
                my_cnt += (uint32_t)__popcll(mk);
            };
            if constexpr (!PAIR) {
                float m = -INFINITY;
#pragma unroll
                for (int j = 0; j < QB; ++j)
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        m = jmax3(m, acc[rb][j][0], acc[rb][j][1]);
                        m = jmax3(m, acc[rb][j][2], acc[rb][j][3]);
                    }
                if (__builtin_amdgcn_ballot_w64(m >= thr) == 0ull) continue;
                // rare off the diagonal; only THIS wave pays for it
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const uint32_t pos_b = col0 + (uint32_t)(16 * j + c16);
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        const float mrb = fmaxf(fmaxf(acc[rb][j][0], acc[rb][j][1]), fmaxf(acc[rb][j][2], acc[rb][j][3]));
                        if (__builtin_amdgcn_ballot_w64(mrb >= thr) == 0ull) continue;  // wave-uniform
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            const float key = acc[rb][j][jj];
                            const uint32_t pos_a = row0 + (uint32_t)(16 * rb + 4 * kg + jj);
                            append(key >= thr && pos_a < pos_b && pos_b < n_rows, pos_a, pos_b, key);
                        }
                    }
                }
            } else {
                // The transformed key of row (rb, jj) against column c16 of block j.  The column's scalars come from the LDS
                // where they are used (one ds_read per 8 keys): QB or 2 QB more registers held across the MFMAs do not fit
                // next to the accumulators and the A fragments at stride 384.  The common path keeps only the maximum; the
                // candidate path forms the keys again -- from a copy of e32 the compiler cannot see through, or it would keep
                // the common path's 64 keys for it -- so no key array is live across the branch.
                auto pair_key = [&](int rb, int j, int jj, float e, float nbc) -> float {
                    return join_pair_key<METRIC>(acc[rb][j][jj], e, ra[rb][jj], nbc);
                };
                float m = -INFINITY;
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const float nbc = col_n[16 * j + c16];
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        m = jmax3(m, pair_key(rb, j, 0, e32, nbc), pair_key(rb, j, 1, e32, nbc));
                        m = jmax3(m, pair_key(rb, j, 2, e32, nbc), pair_key(rb, j, 3, e32, nbc));
                    }
                }
                if (__builtin_amdgcn_ballot_w64(m >= thr) == 0ull) continue;
                float e_again = e32;
                asm volatile("" : "+s"(e_again));
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const uint32_t pos_b = col0 + (uint32_t)(16 * j + c16);
                    const float nbc = col_n[16 * j + c16];
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        const float k0 = pair_key(rb, j, 0, e_again, nbc), k1 = pair_key(rb, j, 1, e_again, nbc);
                        const float k2 = pair_key(rb, j, 2, e_again, nbc), k3 = pair_key(rb, j, 3, e_again, nbc);
                        if (__builtin_amdgcn_ballot_w64(fmaxf(fmaxf(k0, k1), fmaxf(k2, k3)) >= thr) == 0ull) continue;  // wave-uniform
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            const float tk = jj == 0 ? k0 : (jj == 1 ? k1 : (jj == 2 ? k2 : k3));
                            const uint32_t pos_a = row0 + (uint32_t)(16 * rb + 4 * kg + jj);
                            append(tk >= thr && pos_a < pos_b && pos_b < n_rows, pos_a, pos_b, acc[rb][j][jj]);
                        }
                    }
                }
            }
        }
    }
    if (my_cnt) flush_wave();
}

// a counter is cleared by a kernel (nothing here is a memset node, so a launch sequence can be captured as it is)
__global__ void k_join_clear(uint32_t* __restrict__ cnt)
{
    if (threadIdx.x == 0) *cnt = 0u;
}

struct RowsArgs {
    const void* slab;
    uint32_t n_rows, y0, y1;
    float thr;
    JoinCand* cand;
    uint32_t* cnt;
    uint32_t cap, grid;
    const float* row_norm;
    float e32;
};

template <int KSTEPS, int METRIC>
hipError_t launch_rows(hipStream_t s, const RowsArgs& a)
{
    hipLaunchKernelGGL(k_join_clear, dim3(1), dim3(64), 0, s, a.cnt);
    hipLaunchKernelGGL((k_join_rows<KSTEPS, METRIC>), dim3(a.grid), dim3(JOIN_NW * 64), 0, s,
                       reinterpret_cast<const unsigned char*>(a.slab), a.n_rows, a.y0, a.y1, a.thr, a.cand, a.cnt, a.cap, a.row_norm,
                       a.e32);
    return hipGetLastError();
}

template <int METRIC>
hipError_t launch_rows_ldb(hipStream_t s, uint32_t ldb, const RowsArgs& a)
{
    switch (ldb) {
    case 128: return launch_rows<8, METRIC>(s, a);
    case 256: return launch_rows<16, METRIC>(s, a);
    case 384: return launch_rows<24, METRIC>(s, a);
    case 512: return launch_rows<32, METRIC>(s, a);
    default: return launch_rows<48, METRIC>(s, a);
    }
}

}  // namespace

bool join_rows_supported(uint32_t dim, int metric)
{
    const uint32_t ldb = mfma_ldb(dim);
    if (metric != COSINE && metric != EUCLIDEAN && metric != DOT) return false;
    return dim >= 1 && (ldb == 128 || ldb == 256 || ldb == 384 || ldb == 512 || ldb == 768) && mfma_rows_kernel(dim);
}

hipError_t launch_join_rows(hipStream_t s, int metric, const void* slab_frag, const float* row_norm, uint64_t n_rows, uint32_t dim,
                            uint32_t y0, uint32_t y1, float thr, JoinCand* cand, uint32_t* cnt, uint32_t cap, JoinLaunchInfo* info)
{
    if (!join_rows_supported(dim, metric) || n_rows < 2 || n_rows >= 0x7FFFFFFFull || cap == 0) return hipErrorInvalidValue;
    if (metric != COSINE && !row_norm) return hipErrorInvalidValue;
    const uint32_t ldb = mfma_ldb(dim);
    const JoinPlan plan = join_plan((uint32_t)n_rows, join_qpb(ldb));
    if (y0 >= y1 || y1 > plan.n_panels) return hipErrorInvalidValue;
    const uint64_t units = join_units_before(plan, y1) - join_units_before(plan, y0);
    // one workgroup per CU (the panel fills its LDS); at least one wave's worth of blocks per workgroup
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint64_t want = (units + JOIN_NW - 1) / JOIN_NW;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cus, want));
    if (info) {
        info->ksteps = (int)(ldb / 16);
        info->grid = (int)grid;
        info->units = units;
    }
    const RowsArgs a{slab_frag, (uint32_t)n_rows, y0, y1, thr, cand, cnt, cap, grid, row_norm, join_pair_e32(ldb)};
    switch (metric) {
    case COSINE: return launch_rows_ldb<COSINE>(s, ldb, a);
    case EUCLIDEAN: return launch_rows_ldb<EUCLIDEAN>(s, ldb, a);
    default: return launch_rows_ldb<DOT>(s, ldb, a);
    }
}

}  // namespace vl
