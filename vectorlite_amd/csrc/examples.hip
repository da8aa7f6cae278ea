// examples.hip -- exact search by positive and negative examples.
//
// k_examples_rows<KSTEPS, METRIC> is the candidate pass: one launch over every row on the matrix cores
// (v_mfma_f32_16x16x32_bf16) whose epilogue reduces ACROSS the example dimension of the MFMA tile, inside the wave, so that
// a row leaves the kernel as two floats.
//   B = the examples, in 16-column blocks that are all positive or all negative (at most 4 + 2), copied once per workgroup
//       into the padded LDS image k_mfma_rows keeps its queries in (row stride + 32 bytes: conflict-free ds_read_b128).
//       Only the blocks in use are copied and multiplied: their number is a wave-uniform run-time value that selects one of
//       six unrolled bodies, so a one-example call issues one block's MFMAs.
//   A = the waves' own 32-row blocks of the fragment-major slab: one contiguous 1 KB nontemporal load per fragment (a row
//       is read once per call), held for a K phase (the whole K up to stride 256, phases of four K steps above) and
//       refilled right behind its last use with the wave's next block.
//   C = a 32 x (16 blocks) tile per wave.  The keys are k_mfma_rows' keys (cosine: the sum; dot: the sum times the row's
//       norm; Euclidean: 2 sum norm - sqnorm), so the bound's input term IN_EXTRA_MFMA holds unchanged.
// Epilogue: every key goes through its column's (a, c) pair (examples_plan.hpp) onto a scale shared by the examples, a lane
// folds the blocks of a side into 8 running maxima (its 2 x 4 rows), four DPP steps take the maximum over the 16 column
// lanes, and the column-0 lanes store K[row] = (Kp, Kn).  No candidate ring, no threshold, no atomic.
//
// The kernels behind it: k_examples_seed / k_examples_top (the 64 rows of largest estimated f), k_examples_exact (f of a
// list of rows in the reference's order), k_examples_survivors (U >= L), k_examples_rank, and the exact route's fold / fuse.
#include "examples.hpp"

#include <type_traits>

#include "device_common.hpp"
#include "maxsim_plan.hpp"
#include "mfma_scan.hpp"
#include "xcd_map.hpp"

namespace vl {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {
using namespace dev;

constexpr int EX_NW = 8;  // waves per workgroup (two per SIMD)

// the maximum over the 16 lanes of a DPP row (the 16 example columns of a C tile): xor 1, xor 2, then the two mirrors
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_max16(float v)
{
    v = fmaxf(v, dpp_move<0xB1>(v));   // quad_perm [1, 0, 3, 2]
    v = fmaxf(v, dpp_move<0x4E>(v));   // quad_perm [2, 3, 0, 1]
    v = fmaxf(v, dpp_move<0x141>(v));  // row_half_mirror: the other quad of the half row
    v = fmaxf(v, dpp_move<0x140>(v));  // row_mirror: the other half row
    return v;
}

template <int KSTEPS, int METRIC>
__global__ __launch_bounds__(EX_NW * 64) void k_examples_rows(const unsigned char* __restrict__ slab, const float* __restrict__ row_nrm,
                                                              const float* __restrict__ row_sqn,
                                                              const unsigned char* __restrict__ q16,
                                                              const ExamplesMap* __restrict__ map, uint32_t pos_blocks,
                                                              uint32_t n_blocks_ex, uint32_t n_rows, float2* __restrict__ K)
{
    constexpr int LDB = KSTEPS * 16;
    constexpr int ROW_BYTES = LDB * 2;
    constexpr int LDS_ROW = ROW_BYTES + 32;
    constexpr int KS32 = KSTEPS / 2;             // K = 32 per MFMA
    constexpr int MAXB = (int)EXAMPLES_MAX_BLOCKS;
    // K phases of 4 steps above stride 256 (384: 3, 512: 4, 768: 6).  The compiler's resource report decided it: with six
    // example blocks of accumulators next to them, 12 steps of fragments (the whole K at stride 384) spilled 128 bytes and
    // 6-step phases at stride 768 spilled 12; 4-step phases leave every shape without scratch
    constexpr int PH = KS32 > 8 ? KS32 / 4 : 1;
    constexpr int KSP = KS32 / PH;               // A fragments a wave holds per 16-row half block
    constexpr int GROUP_BYTES = 16 * ROW_BYTES;  // one 16-row group of the slab: KS32 chunks of 1 KB
    static_assert(KS32 % PH == 0, "whole K phases");
    static_assert(MAXB * 16 * LDS_ROW + MAXB * 16 * (int)sizeof(ExamplesMap) <= 160 * 1024, "the examples fit the LDS");

    __shared__ __attribute__((aligned(16))) unsigned char q_lds[MAXB * 16 * LDS_ROW];
    __shared__ ExamplesMap map_lds[MAXB * 16];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, kg = lane >> 4;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    const uint32_t nbe = n_blocks_ex < (uint32_t)MAXB ? n_blocks_ex : (uint32_t)MAXB;
    // neighbouring row blocks on one XCD (xcd_map.hpp; a single example chunk: ny = 1)
    uint32_t bx, by;
    xcd_pair(blockIdx.x, gridDim.x, 1u, bx, by);

    // ---- the blocks in use -> LDS (the kernel's only barrier) ----
    {
        constexpr int CPR = ROW_BYTES / 16;
        const int pieces = (int)nbe * 16 * CPR;
        for (int c = tid; c < pieces; c += EX_NW * 64) {
            const int r = c / CPR, cc = c % CPR;
            *reinterpret_cast<u32x4*>(&q_lds[r * LDS_ROW + cc * 16]) = *reinterpret_cast<const u32x4*>(q16 + (size_t)c * 16);
        }
        for (int c = tid; c < (int)nbe * 16; c += EX_NW * 64) map_lds[c] = map[c];
    }
    __syncthreads();

    const uint32_t n_blocks = (n_rows + 31u) / 32u;
    const uint32_t stride = gridDim.x * EX_NW;
    uint32_t b = bx + gridDim.x * (uint32_t)wave;
    if (b >= n_blocks) return;  // wave-uniform; no barrier follows
    const uint32_t b_last = b + ((n_blocks - 1 - b) / stride) * stride;  // a valid block to re-read at the tail

    auto a_ptr = [&](uint32_t blk) { return slab + (size_t)blk * (2 * GROUP_BYTES) + lane_off; };
    auto load_frag = [](const unsigned char* p) { return __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p)); };
    bf16x8 afrag[2][KSP];
    {
        const unsigned char* p = a_ptr(b);
#pragma unroll
        for (int s = 0; s < KSP; ++s)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) afrag[rb][s] = load_frag(p + rb * GROUP_BYTES + s * 1024);
    }
    const unsigned char* qrow = &q_lds[c16 * LDS_ROW + kg * 16];

    // one row block with NB example blocks (compile time: every register index below is static)
    auto block = [&](auto nb_tag, uint32_t blk, uint32_t nxt) {
        constexpr int NB = decltype(nb_tag)::value;
        const unsigned char* pn = a_ptr(nxt);
        const unsigned char* pc = a_ptr(blk);
        const uint32_t row0 = blk * 32u;

        f32x4 acc[2][NB];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ph = 0; ph < PH; ++ph) {
            // the fragments are refilled behind their last use: with this block's next K phase, or the next block's first
            const unsigned char* psrc = ph + 1 < PH ? pc + (size_t)(ph + 1) * KSP * 1024 : pn;
#pragma unroll
            for (int s = 0; s < KSP; ++s) {
                const unsigned char* bp = qrow + (ph * KSP + s) * 64;
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const bf16x8 bq = *reinterpret_cast<const bf16x8*>(bp + j * 16 * LDS_ROW);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[0][s], bq, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[1][s], bq, acc[1][j], 0, 0, 0);
                }
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) afrag[rb][s] = load_frag(psrc + rb * GROUP_BYTES + s * 1024);
                // one K step at a time: left alone the scheduler hoists the example fragments of every step (NB x KSP x 4
                // registers) in front of the first MFMA and spills
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- epilogue: C layout of a 16x16 block: column = lane & 15 (example), row = 4 (lane >> 4) + reg ----
        const bool has_neg = pos_blocks < (uint32_t)NB;  // wave-uniform
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const uint32_t r0 = row0 + (uint32_t)(16 * rb + 4 * kg);  // this lane's 4 rows
            // the per-row scalars (the arrays are allocated in whole 64-row tiles)
            f32x4 nrm = f32x4{1.f, 1.f, 1.f, 1.f}, sqn = f32x4{0.f, 0.f, 0.f, 0.f};
            if (METRIC != COSINE) nrm = *reinterpret_cast<const f32x4*>(row_nrm + r0);
            if (METRIC == EUCLIDEAN) sqn = *reinterpret_cast<const f32x4*>(row_sqn + r0);
            float vp[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, vn[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const ExamplesMap m = map_lds[j * 16 + c16];
                const bool positive = (uint32_t)j < pos_blocks;  // wave-uniform
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float key = acc[rb][j][jj];                                     // cosine: x^.q
                    if (METRIC == DOT) key *= nrm[jj];                              // x.q
                    if (METRIC == EUCLIDEAN) key = 2.0f * key * nrm[jj] - sqn[jj];  // |q|^2 - |x - q|^2
                    const float v = examples_mapped(key, m);
                    if (positive) vp[jj] = fmaxf(vp[jj], v);
                    else vn[jj] = fmaxf(vn[jj], v);
                }
                __builtin_amdgcn_sched_barrier(0);  // one block's keys at a time
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                vp[jj] = row_max16(vp[jj]);
                if (has_neg) vn[jj] = row_max16(vn[jj]);
            }
            if (c16 == 0) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    if (r0 + (uint32_t)jj < n_rows) K[r0 + (uint32_t)jj] = make_float2(vp[jj], vn[jj]);
            }
        }
    };

    auto run = [&](auto nb_tag) {
        for (; b < n_blocks; b += stride) block(nb_tag, b, b + stride < n_blocks ? b + stride : b_last);
    };
    switch (nbe) {  // wave-uniform
    case 1: run(std::integral_constant<int, 1>{}); break;
    case 2: run(std::integral_constant<int, 2>{}); break;
    case 3: run(std::integral_constant<int, 3>{}); break;
    case 4: run(std::integral_constant<int, 4>{}); break;
    case 5: run(std::integral_constant<int, 5>{}); break;
    case 6: run(std::integral_constant<int, 6>{}); break;
    default: break;
    }
}

// one thread per image column
__global__ __launch_bounds__(128) void k_examples_map(int metric, const double* __restrict__ q_norms, uint32_t a, uint32_t b,
                                                      ExamplesMap* __restrict__ map, double* __restrict__ q_max)
{
    const uint32_t c = threadIdx.x;
    if (c < 16u * (examples_blocks(a) + examples_blocks(b))) {
        const uint32_t e = examples_col_example(c, a, b);
        map[c] = examples_map(metric, e == ~0u ? 0.0 : q_norms[e], e == ~0u);
    }
    if (c == 0) {
        double m = 0.0;
        for (uint32_t i = 0; i < a; ++i) m = q_norms[i] > m ? q_norms[i] : m;
        *q_max = m;
    }
}

// an f32 reading of f from (Kp, Kn): it only picks the seeds
template <int METRIC>
__device__ __forceinline__ float seed_estimate(float2 k, bool has_neg)
{
    auto score = [](float v) { return METRIC == EUCLIDEAN ? 1.0f / (1.0f + sqrtf(fmaxf(-v, 0.0f))) : v; };
    const float p = score(k.x);
    if (!has_neg) return p;
    const float n = score(k.y);
    return p > n ? p : -(n * n);
}

template <int METRIC>
__global__ __launch_bounds__(1024) void k_examples_seed(const float2* __restrict__ K, uint32_t n_rows, uint32_t has_neg,
                                                        Cand32* __restrict__ lists)
{
    __shared__ Cand32 sh[16 * WAVE];
    TopList<float> L;
    L.init();
    const uint32_t step = gridDim.x * 1024;
    for (uint32_t b0 = blockIdx.x * 1024; b0 < n_rows; b0 += step) {  // workgroup-uniform trip count
        const uint32_t p = b0 + threadIdx.x;
        const bool in = p < n_rows;
        const float est = in ? seed_estimate<METRIC>(K[p], has_neg != 0u) : -INFINITY;
        L.offer(est, p, in);
    }
    block_merge<float, Cand32, 16>(L, sh);
    if ((threadIdx.x >> 6) == 0) {
        Cand32 e;
        e.key = L.key;
        e.pos = L.pos;
        lists[(size_t)blockIdx.x * KP + lane_id()] = e;
    }
}

// The n_lists <= 64 workgroup lists merged into one: top[], ctr[SEEDS]
__global__ __launch_bounds__(1024) void k_examples_top(const Cand32* __restrict__ lists, int n_lists, uint32_t* __restrict__ top,
                                                       uint32_t* __restrict__ ctr)
{
    __shared__ Cand32 sh[16 * WAVE];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    TopList<float> L;
    {
        const int first = wave * 4;
        int c = n_lists - first;
        c = c < 0 ? 0 : (c > 4 ? 4 : c);
        fold_lists4<float, Cand32>(L, lists, first, c);
    }
    block_merge<float, Cand32, 16>(L, sh);
    if (wave == 0) {
        const unsigned long long have = __ballot(L.pos != POS_SENTINEL);  // a prefix of the lanes: the list is sorted
        const uint32_t c = (uint32_t)__popcll(have);
        if ((uint32_t)lane < c) top[lane] = L.pos;
        if (lane == 0) ctr[EXAMPLES_CTR_SEEDS] = c;
    }
}

// the ordered maximum of f64 scores: -0.0 below +0.0 (their encodings differ)
__device__ __forceinline__ double ordered_max(double x, double y) { return maxsim_score_enc(y) > maxsim_score_enc(x) ? y : x; }
// f from the two per-side maxima: one f64 multiply, then the negation
__device__ __forceinline__ double fuse(double P, double N, bool has_neg)
{
    if (!has_neg || P > N) return P;
    const double nn = N * N;
    return -nn;
}

// One wave per listed row; its lanes take the examples (lane, lane + 64), each in the reference's arithmetic (Acc64) in
// index order, and share the row (one broadcast load per column).  Sized for hundreds of rows, not for speed.
template <int METRIC>
__global__ __launch_bounds__(256) void k_examples_exact(const double* __restrict__ master, const double* __restrict__ q64, uint32_t a,
                                                        uint32_t b, uint32_t dim, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ n_list, uint32_t cap, uint32_t n_rows,
                                                        double* __restrict__ f, uint32_t* __restrict__ ctr)
{
    const uint32_t n = *n_list;
    if (n > cap) return;  // the list is incomplete: the host takes the exact route
    const uint32_t lane = (uint32_t)lane_id();
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {  // wave-uniform
        const uint32_t pos = list[i];
        if (pos >= n_rows) continue;
        const double* x = master + (size_t)pos * dim;
        unsigned long long pe = 0ull, ne = 0ull;  // 0 is below every encoding
        for (uint32_t e = lane; e < a + b; e += 64) {
            const double* y = q64 + (size_t)e * dim;
            Acc64<METRIC> A;
            A.init();
            for (uint32_t c = 0; c < dim; ++c) A.step(x[c], y[c]);
            const double sc = A.score();
            if (sc != sc) {
                ctr[EXAMPLES_CTR_NAN] = 1u;
                continue;
            }
            const unsigned long long enc = maxsim_score_enc(sc);
            if (e < a) pe = enc > pe ? enc : pe;
            else ne = enc > ne ? enc : ne;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long po = __shfl_xor(pe, o), no = __shfl_xor(ne, o);
            pe = po > pe ? po : pe;
            ne = no > ne ? no : ne;
        }
        // (a side whose scores are all NaN leaves 0: the flag is set and the call fails)
        if (lane == 0) f[i] = fuse(maxsim_score_dec(pe), maxsim_score_dec(ne), b != 0u);
    }
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_examples_survivors(const float2* __restrict__ K, uint32_t n_rows, uint32_t has_neg,
                                                            uint32_t ldb, double R, const double* __restrict__ q_max, double L,
                                                            uint32_t cap, uint32_t* __restrict__ list, uint32_t* __restrict__ ctr)
{
    const int lane = lane_id();
    const double qm = *q_max;
    const uint32_t step = gridDim.x * 256;
    for (uint32_t b0 = blockIdx.x * 256; b0 < n_rows; b0 += step) {  // wave-uniform trip count
        const uint32_t p = b0 + threadIdx.x;
        // !(U < L): a NaN bound keeps its row
        const bool in = p < n_rows && !(examples_upper<METRIC>(K[p].x, has_neg != 0u, ldb, R, qm, IN_EXTRA_MFMA) < L);
        const unsigned long long mk = __ballot(in);
        if (mk == 0ull) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(ctr + EXAMPLES_CTR_SURVIVORS, (uint32_t)__popcll(mk));
        base = read_lane(base, 0);
        const uint32_t slot = base + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
        if (in && slot < cap) list[slot] = p;
    }
}

// Rank by counting: entry i goes to slot #{j : j in front of i}, in front = higher f, then lower position (two entries'
// positions differ, so the slots are a permutation).  One workgroup; both arrays in LDS.
__global__ __launch_bounds__(1024) void k_examples_rank(const uint32_t* __restrict__ list, const double* __restrict__ f,
                                                        const uint32_t* __restrict__ n_list, uint32_t cap, uint32_t k,
                                                        uint32_t* __restrict__ out_pos, double* __restrict__ out_f)
{
    __shared__ double sc[EXAMPLES_CAND_CAP];
    __shared__ uint32_t ps[EXAMPLES_CAND_CAP];
    const uint32_t n = *n_list;
    if (n > cap || n > EXAMPLES_CAND_CAP) return;  // workgroup-uniform
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        sc[i] = f[i];
        ps[i] = list[i];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        const double si = sc[i];
        const uint32_t pi = ps[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const double sj = sc[j];
            rank += (sj > si || (sj == si && ps[j] < pi)) ? 1u : 0u;
        }
        if (rank < k) {
            out_pos[rank] = pi;
            out_f[rank] = si;
        }
    }
}

// ---- the exact route ----
__global__ __launch_bounds__(256) void k_examples_fold(const double* __restrict__ scores, uint32_t n_rows, uint32_t first,
                                                       double* __restrict__ acc, uint32_t* __restrict__ ctr)
{
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < n_rows; p += gridDim.x * 256) {
        const double sc = scores[p];
        if (sc != sc) {
            ctr[EXAMPLES_CTR_NAN] = 1u;
            continue;
        }
        acc[p] = first ? sc : ordered_max(acc[p], sc);
    }
}
__global__ __launch_bounds__(256) void k_examples_fuse(const double* __restrict__ P, const double* __restrict__ N, uint32_t n_rows,
                                                       double* __restrict__ f)
{
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < n_rows; p += gridDim.x * 256) f[p] = fuse(P[p], N ? N[p] : 0.0, N != nullptr);
}

int grid_for(uint64_t n, int per, int max_grid)
{
    const uint64_t blocks = (n + (uint64_t)per - 1) / (uint64_t)per;
    return (int)(blocks < 1 ? 1 : (blocks < (uint64_t)max_grid ? blocks : (uint64_t)max_grid));
}

template <int KSTEPS, int METRIC>
hipError_t launch_rows(hipStream_t s, int grid, const void* slab, const float* nrm, const float* sqn, const void* q16,
                       const ExamplesMap* map, uint32_t pb, uint32_t nb, uint32_t n_rows, float2* K)
{
    hipLaunchKernelGGL((k_examples_rows<KSTEPS, METRIC>), dim3(grid), dim3(EX_NW * 64), 0, s, reinterpret_cast<const unsigned char*>(slab),
                       nrm, sqn, reinterpret_cast<const unsigned char*>(q16), map, pb, nb, n_rows, K);
    return hipGetLastError();
}

template <int METRIC>
hipError_t launch_rows_ldb(hipStream_t s, uint32_t ldb, int grid, const void* slab, const float* nrm, const float* sqn, const void* q16,
                           const ExamplesMap* map, uint32_t pb, uint32_t nb, uint32_t n_rows, float2* K)
{
    switch (ldb) {
    case 128: return launch_rows<8, METRIC>(s, grid, slab, nrm, sqn, q16, map, pb, nb, n_rows, K);
    case 256: return launch_rows<16, METRIC>(s, grid, slab, nrm, sqn, q16, map, pb, nb, n_rows, K);
    case 384: return launch_rows<24, METRIC>(s, grid, slab, nrm, sqn, q16, map, pb, nb, n_rows, K);
    case 512: return launch_rows<32, METRIC>(s, grid, slab, nrm, sqn, q16, map, pb, nb, n_rows, K);
    default: return launch_rows<48, METRIC>(s, grid, slab, nrm, sqn, q16, map, pb, nb, n_rows, K);
    }
}

bool counts_ok(uint32_t a, uint32_t b) { return a >= 1 && a <= EXAMPLES_MAX_POS && b <= EXAMPLES_MAX_NEG; }

}  // namespace

bool examples_rows_supported(uint32_t dim, int metric)
{
    const uint32_t ldb = mfma_ldb(dim);
    if (metric != COSINE && metric != EUCLIDEAN && metric != DOT) return false;
    return dim >= 1 && (ldb == 128 || ldb == 256 || ldb == 384 || ldb == 512 || ldb == 768) && mfma_rows_kernel(dim);
}

hipError_t launch_examples_map(hipStream_t s, int metric, const double* q_norms, uint32_t a, uint32_t b, ExamplesMap* map,
                               double* q_max)
{
    if (!counts_ok(a, b) || !q_norms || !map || !q_max) return hipErrorInvalidValue;
    static_assert(EXAMPLES_MAX_COLS <= 128, "one thread per image column");
    hipLaunchKernelGGL(k_examples_map, dim3(1), dim3(128), 0, s, metric, q_norms, a, b, map, q_max);
    return hipGetLastError();
}

hipError_t launch_examples_rows(hipStream_t s, int metric, const void* slab_frag, const float* row_norm, const float* row_sqnorm,
                                const void* q_bf16, const ExamplesMap* map, uint32_t a, uint32_t b, uint64_t n_rows, uint32_t dim,
                                float2* K, ExamplesRowsInfo* info)
{
    if (!examples_rows_supported(dim, metric) || n_rows == 0 || n_rows >= 0xFFFFFFE0ull || !counts_ok(a, b) || !slab_frag || !q_bf16 ||
        !map || !K)
        return hipErrorInvalidValue;
    if (metric != COSINE && (!row_norm || (metric == EUCLIDEAN && !row_sqnorm))) return hipErrorInvalidValue;
    const uint32_t ldb = mfma_ldb(dim);
    const uint32_t pb = examples_blocks(a), nb = pb + examples_blocks(b);
    // one workgroup per CU (the examples may fill its LDS); at least one 32-row block per wave
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint64_t n_blocks = (n_rows + 31) / 32;
    const int gx = grid_for(n_blocks, EX_NW, cus > 0 ? cus : 256);
    if (info) {
        info->ksteps = (int)(ldb / 16);
        info->blocks = (int)nb;
        info->grid_x = gx;
    }
    switch (metric) {
    case COSINE: return launch_rows_ldb<COSINE>(s, ldb, gx, slab_frag, row_norm, row_sqnorm, q_bf16, map, pb, nb, (uint32_t)n_rows, K);
    case EUCLIDEAN:
        return launch_rows_ldb<EUCLIDEAN>(s, ldb, gx, slab_frag, row_norm, row_sqnorm, q_bf16, map, pb, nb, (uint32_t)n_rows, K);
    default: return launch_rows_ldb<DOT>(s, ldb, gx, slab_frag, row_norm, row_sqnorm, q_bf16, map, pb, nb, (uint32_t)n_rows, K);
    }
}

hipError_t launch_examples_seed(hipStream_t s, int metric, const float2* K, uint64_t n_rows, bool has_neg, Cand32* lists,
                                uint32_t* top, uint32_t* ctr)
{
    if (n_rows == 0 || n_rows >= 0xFFFFFFE0ull) return hipErrorInvalidValue;
    const int grid = grid_for(n_rows, 1024, EXAMPLES_TOP_LISTS);
    const uint32_t n = (uint32_t)n_rows, hn = has_neg ? 1u : 0u;
    switch (metric) {
    case COSINE: hipLaunchKernelGGL(k_examples_seed<COSINE>, dim3(grid), dim3(1024), 0, s, K, n, hn, lists); break;
    case EUCLIDEAN: hipLaunchKernelGGL(k_examples_seed<EUCLIDEAN>, dim3(grid), dim3(1024), 0, s, K, n, hn, lists); break;
    case DOT: hipLaunchKernelGGL(k_examples_seed<DOT>, dim3(grid), dim3(1024), 0, s, K, n, hn, lists); break;
    default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_examples_top, dim3(1), dim3(1024), 0, s, (const Cand32*)lists, grid, top, ctr);
    return hipGetLastError();
}

hipError_t launch_examples_exact(hipStream_t s, int metric, const double* master, const double* q64, uint32_t a, uint32_t b,
                                 uint32_t dim, const uint32_t* list, const uint32_t* n_list, uint32_t cap, uint64_t n_rows,
                                 double* f, uint32_t* ctr)
{
    if (n_rows == 0 || n_rows >= 0xFFFFFFFFull || !counts_ok(a, b) || cap == 0 || cap > EXAMPLES_CAND_CAP) return hipErrorInvalidValue;
    const int grid = grid_for(cap, 4, 2048);  // grid-stride over the device's own count
    const uint32_t n = (uint32_t)n_rows;
    switch (metric) {
    case COSINE: hipLaunchKernelGGL(k_examples_exact<COSINE>, dim3(grid), dim3(256), 0, s, master, q64, a, b, dim, list, n_list, cap, n, f, ctr); break;
    case EUCLIDEAN:
        hipLaunchKernelGGL(k_examples_exact<EUCLIDEAN>, dim3(grid), dim3(256), 0, s, master, q64, a, b, dim, list, n_list, cap, n, f, ctr);
        break;
    case DOT: hipLaunchKernelGGL(k_examples_exact<DOT>, dim3(grid), dim3(256), 0, s, master, q64, a, b, dim, list, n_list, cap, n, f, ctr); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_examples_survivors(hipStream_t s, int metric, const float2* K, uint64_t n_rows, bool has_neg, uint32_t ldb,
                                     double R, const double* q_max, double L, uint32_t cap, uint32_t* list, uint32_t* ctr)
{
    if (n_rows == 0 || n_rows >= 0xFFFFFFE0ull || cap == 0 || cap > EXAMPLES_CAND_CAP) return hipErrorInvalidValue;
    const int grid = grid_for(n_rows, 256, 2048);
    const uint32_t n = (uint32_t)n_rows, hn = has_neg ? 1u : 0u;
    switch (metric) {
    case COSINE: hipLaunchKernelGGL(k_examples_survivors<COSINE>, dim3(grid), dim3(256), 0, s, K, n, hn, ldb, R, q_max, L, cap, list, ctr); break;
    case EUCLIDEAN:
        hipLaunchKernelGGL(k_examples_survivors<EUCLIDEAN>, dim3(grid), dim3(256), 0, s, K, n, hn, ldb, R, q_max, L, cap, list, ctr);
        break;
    case DOT: hipLaunchKernelGGL(k_examples_survivors<DOT>, dim3(grid), dim3(256), 0, s, K, n, hn, ldb, R, q_max, L, cap, list, ctr); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_examples_rank(hipStream_t s, const uint32_t* list, const double* f, const uint32_t* n_list, uint32_t cap,
                                uint32_t k, uint32_t* out_pos, double* out_f)
{
    if (cap == 0 || cap > EXAMPLES_CAND_CAP || k == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_examples_rank, dim3(1), dim3(1024), 0, s, list, f, n_list, cap, k, out_pos, out_f);
    return hipGetLastError();
}

hipError_t launch_examples_fold(hipStream_t s, const double* scores, uint64_t n_rows, bool first, double* acc, uint32_t* ctr)
{
    if (n_rows == 0 || n_rows >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_examples_fold, dim3(grid_for(n_rows, 256, 4096)), dim3(256), 0, s, scores, (uint32_t)n_rows, first ? 1u : 0u, acc,
                       ctr);
    return hipGetLastError();
}

hipError_t launch_examples_fuse(hipStream_t s, const double* P, const double* N, uint64_t n_rows, double* f)
{
    if (n_rows == 0 || n_rows >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_examples_fuse, dim3(grid_for(n_rows, 256, 4096)), dim3(256), 0, s, P, N, (uint32_t)n_rows, f);
    return hipGetLastError();
}

}  // namespace vl
