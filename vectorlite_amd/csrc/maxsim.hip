// maxsim.hip -- late-interaction (MaxSim) search over grouped rows.
//
// k_maxsim_rows<KSTEPS, METRIC> is the candidate pass: one launch over every row on the matrix cores
// (v_mfma_f32_16x16x32_bf16), with a SEGMENTED MAX as its epilogue.
//   B = the query's tokens, a chunk of maxsim_qpb(stride) of them (128; 96 at stride 768) copied once per workgroup into the
//       padded LDS image k_mfma_rows keeps its queries in (row stride + 32 bytes: conflict-free ds_read_b128).
//   A = the waves' own 32-row blocks of the fragment-major slab: one contiguous 1 KB load per fragment, held for a K phase
//       (the whole K up to stride 384, four phases at 512 and 768) and refilled right behind its last use with the wave's
//       next block.
//   C = a 32 x chunk tile per wave.  The keys are k_mfma_rows' keys (cosine: the sum; dot: the sum times the row's norm;
//       Euclidean: 2 sum norm - sqnorm), so the bound's input term IN_EXTRA_MFMA holds unchanged.
// The epilogue has no threshold and no ring: it raises M[token][group], a table of ordered f32 keys.  A lane owns 4
// consecutive rows of a 16-row block and fetches their groups with one 16-byte load.  When the whole 16-row block is one
// group (a ballot) the maximum runs over the lane's 4 rows, then across the four lanes of a column, and the kg == 0 lanes
// issue ONE atomicMax per token: 16 x chunk/16 atomics per 16 rows.  Otherwise a lane merges runs of equal neighbours among
// its 4 rows and issues one atomic per run.  Either way the slot is read first and the atomic skipped when it would not
// raise it (a stale read is only ever too small: the slots never fall).
//
// The kernels behind it: k_maxsim_upper (the per-group upper bound U and the 64 largest), k_maxsim_survivors, and
// k_maxsim_members / k_maxsim_exact / k_maxsim_sum, which score a list of groups exactly in the reference's order.
#include "maxsim.hpp"

#include "device_common.hpp"
#include "mfma_scan.hpp"

namespace vl {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {
using namespace dev;

constexpr int MS_NW = 8;  // waves per workgroup (two per SIMD)

// raise *slot to enc unless it is there already
__device__ __forceinline__ void raise_slot(uint32_t* slot, uint32_t enc)
{
    if (__atomic_load_n(slot, __ATOMIC_RELAXED) < enc) atomicMax(slot, enc);
}

template <int KSTEPS, int METRIC>
__global__ __launch_bounds__(MS_NW * 64) void k_maxsim_rows(const unsigned char* __restrict__ slab, const float* __restrict__ row_nrm,
                                                            const float* __restrict__ row_sqn,
                                                            const unsigned char* __restrict__ q16, uint32_t n_tokens,
                                                            uint32_t n_rows, const uint32_t* __restrict__ group_of_row,
                                                            uint32_t n_groups, uint32_t* __restrict__ M)
{
    constexpr int LDB = KSTEPS * 16;
    constexpr int ROW_BYTES = LDB * 2;
    constexpr int LDS_ROW = ROW_BYTES + 32;
    constexpr int KS32 = KSTEPS / 2;               // K = 32 per MFMA
    constexpr int QPB = (int)maxsim_qpb((uint32_t)LDB);
    constexpr int QB = QPB / 16;                   // token blocks of the chunk
    constexpr int PH = KS32 > 12 ? 4 : 1;          // K phases: 16 = 4 x 4 (stride 512), 24 = 4 x 6 (stride 768)
    constexpr int KSP = KS32 / PH;                 // A fragments a wave holds per 16-row half block
    constexpr int GROUP_BYTES = 16 * ROW_BYTES;    // one 16-row group of the slab: KS32 chunks of 1 KB
    static_assert(KS32 % PH == 0, "whole K phases");
    static_assert(QPB * LDS_ROW <= 160 * 1024, "the token chunk fits the LDS");

    __shared__ __attribute__((aligned(16))) unsigned char q_lds[QPB * LDS_ROW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, kg = lane >> 4;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    const uint32_t chunk_base = blockIdx.y * (uint32_t)QPB;

    // ---- this chunk's tokens -> LDS (the kernel's only barrier); the bf16 image is padded to whole chunks ----
    {
        constexpr int CPR = ROW_BYTES / 16;
        constexpr int PIECES = QPB * CPR;
        const unsigned char* src = q16 + (size_t)chunk_base * ROW_BYTES;
        for (int c = tid; c < PIECES; c += MS_NW * 64) {
            const int r = c / CPR, cc = c % CPR;
            *reinterpret_cast<u32x4*>(&q_lds[r * LDS_ROW + cc * 16]) = *reinterpret_cast<const u32x4*>(src + (size_t)c * 16);
        }
    }
    __syncthreads();

    const uint32_t n_blocks = (n_rows + 31u) / 32u;
    const uint32_t stride = gridDim.x * MS_NW;
    uint32_t b = blockIdx.x + gridDim.x * (uint32_t)wave;
    if (b >= n_blocks) return;  // wave-uniform; no barrier follows
    const uint32_t b_last = b + ((n_blocks - 1 - b) / stride) * stride;  // a valid block to re-read at the tail

    auto a_ptr = [&](uint32_t blk) { return slab + (size_t)blk * (2 * GROUP_BYTES) + lane_off; };
    bf16x8 afrag[2][KSP];
    {
        const unsigned char* p = a_ptr(b);
#pragma unroll
        for (int s = 0; s < KSP; ++s)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) afrag[rb][s] = *reinterpret_cast<const bf16x8*>(p + rb * GROUP_BYTES + s * 1024);
    }
    const unsigned char* qrow = &q_lds[c16 * LDS_ROW + kg * 16];

    for (; b < n_blocks; b += stride) {
        const uint32_t nxt = b + stride < n_blocks ? b + stride : b_last;
        const unsigned char* pn = a_ptr(nxt);
        const unsigned char* pc = a_ptr(b);
        const uint32_t row0 = b * 32u;

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
                const unsigned char* bp = qrow + (ph * KSP + s) * 64;
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const bf16x8 bq = *reinterpret_cast<const bf16x8*>(bp + j * 16 * LDS_ROW);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[0][s], bq, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[1][s], bq, acc[1][j], 0, 0, 0);
                }
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) afrag[rb][s] = *reinterpret_cast<const bf16x8*>(psrc + rb * GROUP_BYTES + s * 1024);
            }
        }

        // ---- epilogue: C layout of a 16x16 block: column = lane & 15 (token), row = 4 (lane >> 4) + reg ----
        const bool partial = row0 + 32u > n_rows;  // wave-uniform: only the last block holds rows past the end
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const uint32_t r0 = row0 + (uint32_t)(16 * rb + 4 * kg);  // this lane's 4 rows
            // the rows' groups: one 16-byte load (group_of_row holds n_rows words: the last block is read word by word)
            u32x4 g;
            if (!partial) {
                g = *reinterpret_cast<const u32x4*>(group_of_row + r0);
            } else {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) g[jj] = r0 + (uint32_t)jj < n_rows ? group_of_row[r0 + (uint32_t)jj] : MAXSIM_NO_CAND;
            }
            // the per-row scalars (the arrays are allocated in whole 64-row tiles)
            f32x4 nrm = f32x4{1.f, 1.f, 1.f, 1.f}, sqn = f32x4{0.f, 0.f, 0.f, 0.f};
            if (METRIC != COSINE) nrm = *reinterpret_cast<const f32x4*>(row_nrm + r0);
            if (METRIC == EUCLIDEAN) sqn = *reinterpret_cast<const f32x4*>(row_sqn + r0);
            auto key_of = [&](int j, int jj) -> float {
                float key = acc[rb][j][jj];                                           // cosine: x^.q
                if (METRIC == DOT) key *= nrm[jj];                                    // x.q
                if (METRIC == EUCLIDEAN) key = 2.0f * key * nrm[jj] - sqn[jj];        // |q|^2 - |x - q|^2
                return key;
            };
            const uint32_t g0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g[0]);
            const bool same = g[0] == g0 && g[1] == g0 && g[2] == g0 && g[3] == g0;
            if (__builtin_amdgcn_ballot_w64(same) == ~0ull) {  // the 16-row block is one group (or has none)
                if (g0 >= n_groups) continue;                  // rows without a group take no part
                uint32_t* Mg = M + g0;
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    float m = fmaxf(fmaxf(key_of(j, 0), key_of(j, 1)), fmaxf(key_of(j, 2), key_of(j, 3)));
                    m = fmaxf(m, __shfl_xor(m, 16));  // the four kg lanes of a column hold the block's other rows
                    m = fmaxf(m, __shfl_xor(m, 32));
                    const uint32_t token = chunk_base + (uint32_t)(16 * j + c16);
                    if (kg == 0 && token < n_tokens) raise_slot(Mg + (size_t)token * n_groups, maxsim_key_enc(m));
                }
            } else {
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const uint32_t token = chunk_base + (uint32_t)(16 * j + c16);
                    if (token >= n_tokens) continue;  // padding tokens have no row in M
                    uint32_t* Mt = M + (size_t)token * n_groups;
                    // runs of equal neighbours among the lane's 4 rows: one atomic per run
                    uint32_t cg = g[0];
                    float cm = key_of(j, 0);
#pragma unroll
                    for (int jj = 1; jj < 4; ++jj) {
                        const float kj = key_of(j, jj);
                        if (g[jj] == cg) {
                            cm = fmaxf(cm, kj);
                        } else {
                            if (cg < n_groups) raise_slot(Mt + cg, maxsim_key_enc(cm));
                            cg = g[jj];
                            cm = kj;
                        }
                    }
                    if (cg < n_groups) raise_slot(Mt + cg, maxsim_key_enc(cm));
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_maxsim_fill(uint32_t* __restrict__ p, unsigned long long n, uint32_t v)
{
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) p[i] = v;
}
__global__ __launch_bounds__(256) void k_maxsim_fill64(unsigned long long* __restrict__ p, unsigned long long n, unsigned long long v)
{
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) p[i] = v;
}

// U[g] and the per-workgroup top-64 lists of (U, g); one thread per group, the table read along g (coalesced)
template <int METRIC>
__global__ __launch_bounds__(1024) void k_maxsim_upper(const uint32_t* __restrict__ M, uint32_t n_tokens, uint32_t n_groups,
                                                       uint32_t ldb, double R, const double* __restrict__ q_norms,
                                                       double* __restrict__ U, Cand64* __restrict__ lists,
                                                       uint32_t* __restrict__ ctr)
{
    __shared__ Cand64 sh[16 * WAVE];
    TopList<double> L;
    L.init();
    const uint32_t step = gridDim.x * 1024;
    uint32_t mine = 0;
    for (uint32_t b0 = blockIdx.x * 1024; b0 < n_groups; b0 += step) {  // workgroup-uniform trip count
        const uint32_t g = b0 + threadIdx.x;
        bool has = false;
        double u = -(double)INFINITY;
        if (g < n_groups) {
            has = M[g] != MAXSIM_KEY_NEG_INF;  // every row of a group raises every token's slot above -inf
            if (has) {
                u = maxsim_term_up(bound_for_key<METRIC>(maxsim_key_dec(M[g]), ldb, R, q_norms[0], IN_EXTRA_MFMA), n_tokens);
                for (uint32_t t = 1; t < n_tokens; ++t)
                    u = u + maxsim_term_up(bound_for_key<METRIC>(maxsim_key_dec(M[(size_t)t * n_groups + g]), ldb, R, q_norms[t],
                                                                 IN_EXTRA_MFMA),
                                           n_tokens);
            }
            U[g] = u;
        }
        mine += (uint32_t)__popcll(__ballot(has));
        L.offer(u, g, has);
    }
    if (lane_id() == 0 && mine) atomicAdd(ctr + MAXSIM_CTR_GROUPS, mine);
    block_merge<double, Cand64, 16>(L, sh);
    if ((threadIdx.x >> 6) == 0) {
        Cand64 e;
        e.key = L.key;
        e.pos = L.pos;
        e.pad = 0;
        lists[(size_t)blockIdx.x * KP + lane_id()] = e;
    }
}

// The n_lists <= 64 workgroup lists merged into one: top[], flag[], ctr[TOP]
__global__ __launch_bounds__(1024) void k_maxsim_top(const Cand64* __restrict__ lists, int n_lists, uint32_t* __restrict__ top,
                                                     uint32_t* __restrict__ flag, uint32_t* __restrict__ ctr)
{
    __shared__ Cand64 sh[16 * WAVE];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    TopList<double> L;
    {
        const int first = wave * 4;
        int c = n_lists - first;
        c = c < 0 ? 0 : (c > 4 ? 4 : c);
        fold_lists4<double, Cand64>(L, lists, first, c);
    }
    block_merge<double, Cand64, 16>(L, sh);
    if (wave == 0) {
        const unsigned long long have = __ballot(L.pos != POS_SENTINEL);  // a prefix of the lanes: the list is sorted
        const uint32_t c = (uint32_t)__popcll(have);
        if ((uint32_t)lane < c) {
            top[lane] = L.pos;
            flag[L.pos] = (uint32_t)lane;
        }
        if (lane == 0) ctr[MAXSIM_CTR_TOP] = c;
    }
}

__global__ __launch_bounds__(256) void k_maxsim_survivors(const double* __restrict__ U, uint32_t n_groups, double L, uint32_t cap,
                                                          uint32_t* __restrict__ list, uint32_t* __restrict__ flag,
                                                          uint32_t* __restrict__ ctr)
{
    const int lane = lane_id();
    const uint32_t step = gridDim.x * 256;
    for (uint32_t b0 = blockIdx.x * 256; b0 < n_groups; b0 += step) {  // wave-uniform trip count
        const uint32_t g = b0 + threadIdx.x;
        const bool in = g < n_groups && U[g] >= L;  // an empty group's U is -inf, L is a finite score or +-inf of real rows
        const unsigned long long mk = __ballot(in);
        if (mk == 0ull) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(ctr + MAXSIM_CTR_SURVIVORS, (uint32_t)__popcll(mk));
        base = read_lane(base, 0);
        const uint32_t slot = base + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
        if (in && slot < cap) {
            list[slot] = g;
            flag[g] = slot;
        }
    }
}

// (candidate, position) of every row whose group is flagged
__global__ __launch_bounds__(256) void k_maxsim_members(const uint32_t* __restrict__ group_of_row, uint32_t n_rows, uint32_t n_groups,
                                                        const uint32_t* __restrict__ flag, MaxsimMember* __restrict__ members,
                                                        uint32_t row_cap, uint32_t* __restrict__ ctr)
{
    const int lane = lane_id();
    const uint32_t step = gridDim.x * 256;
    for (uint32_t b0 = blockIdx.x * 256; b0 < n_rows; b0 += step) {  // wave-uniform trip count
        const uint32_t p = b0 + threadIdx.x;
        uint32_t ci = MAXSIM_NO_CAND;
        if (p < n_rows) {
            const uint32_t g = group_of_row[p];
            if (g < n_groups) ci = flag[g];
        }
        const bool in = ci != MAXSIM_NO_CAND;
        const unsigned long long mk = __ballot(in);
        if (mk == 0ull) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(ctr + MAXSIM_CTR_MEMBERS, (uint32_t)__popcll(mk));
        base = read_lane(base, 0);
        const uint32_t slot = base + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
        if (in && slot < row_cap) members[slot] = MaxsimMember{ci, p};
    }
}

// One thread per (member, token): the reference's arithmetic (Acc64) in index order, then fetch_max into E.  The threads of
// a wave share a member row (one broadcast load per column) and walk neighbouring tokens.
template <int METRIC>
__global__ __launch_bounds__(256) void k_maxsim_exact(const double* __restrict__ master, const double* __restrict__ q64,
                                                      uint32_t n_tokens, uint32_t dim, const MaxsimMember* __restrict__ members,
                                                      uint32_t row_cap, uint32_t n_rows, uint32_t cand_cap,
                                                      unsigned long long* __restrict__ E, uint32_t* __restrict__ ctr)
{
    const uint32_t n_members = ctr[MAXSIM_CTR_MEMBERS];
    if (n_members > row_cap) return;  // the list is incomplete: the host takes the exact route
    const unsigned long long total = (unsigned long long)n_members * n_tokens;
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < total; i += gridDim.x * 256ull) {
        const MaxsimMember mb = members[i / n_tokens];
        const uint32_t t = (uint32_t)(i % n_tokens);
        if (mb.pos >= n_rows || mb.cand >= cand_cap) continue;
        const double* x = master + (size_t)mb.pos * dim;
        const double* y = q64 + (size_t)t * dim;
        Acc64<METRIC> A;
        A.init();
        for (uint32_t c = 0; c < dim; ++c) A.step(x[c], y[c]);
        const double sc = A.score();
        if (sc != sc) ctr[MAXSIM_CTR_NAN] = 1u;
        else atomicMax(E + (size_t)mb.cand * n_tokens + t, maxsim_score_enc(sc));
    }
}

// score[c] = ((m_0 + m_1) + m_2) + ... of candidate c's row of E, one lane per candidate
__global__ __launch_bounds__(256) void k_maxsim_sum(const unsigned long long* __restrict__ E, uint32_t n_tokens,
                                                    const uint32_t* __restrict__ n_cand, uint32_t cap, double* __restrict__ scores)
{
    const uint32_t n = *n_cand < cap ? *n_cand : cap;
    for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) {
        const unsigned long long* e = E + (size_t)c * n_tokens;
        double s = maxsim_score_dec(e[0]);
        for (uint32_t t = 1; t < n_tokens; ++t) s = s + maxsim_score_dec(e[t]);
        scores[c] = s;
    }
}

// Rank by counting: entry i goes to slot #{j : j in front of i}, in front = higher score, then lower group key (the keys of
// two groups differ, so the slots are a permutation).  One workgroup; both arrays in LDS.
__global__ __launch_bounds__(1024) void k_maxsim_rank(const uint32_t* __restrict__ list, const double* __restrict__ scores,
                                                      const uint32_t* __restrict__ n_cand, uint32_t cap,
                                                      const unsigned long long* __restrict__ group_keys, uint32_t k,
                                                      unsigned long long* __restrict__ out_keys, double* __restrict__ out_scores)
{
    __shared__ double sc[MAXSIM_CAND_CAP];
    __shared__ unsigned long long ky[MAXSIM_CAND_CAP];
    const uint32_t n = *n_cand;
    if (n > cap || n > MAXSIM_CAND_CAP) return;  // workgroup-uniform
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        sc[i] = scores[i];
        ky[i] = group_keys[list[i]];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        const double si = sc[i];
        const unsigned long long ki = ky[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const double sj = sc[j];
            rank += (sj > si || (sj == si && ky[j] < ki)) ? 1u : 0u;
        }
        if (rank < k) {
            out_keys[rank] = ki;
            out_scores[rank] = si;
        }
    }
}

// ---- the exact route ----
__global__ __launch_bounds__(256) void k_maxsim_segmax(const double* __restrict__ scores, const uint32_t* __restrict__ group_of_row,
                                                       uint32_t n_rows, uint32_t n_groups, unsigned long long* __restrict__ E1,
                                                       uint32_t* __restrict__ ctr)
{
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < n_rows; p += gridDim.x * 256) {
        const uint32_t g = group_of_row[p];
        if (g >= n_groups) continue;
        const double sc = scores[p];
        if (sc != sc) {
            ctr[MAXSIM_CTR_NAN] = 1u;
            continue;
        }
        const unsigned long long enc = maxsim_score_enc(sc);
        if (__atomic_load_n(E1 + g, __ATOMIC_RELAXED) < enc) atomicMax(E1 + g, enc);
    }
}
__global__ __launch_bounds__(256) void k_maxsim_acc(unsigned long long* __restrict__ E1, double* __restrict__ acc, uint32_t n_groups,
                                                    uint32_t first)
{
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < n_groups; g += gridDim.x * 256) {
        const unsigned long long e = E1[g];
        E1[g] = 0ull;
        if (e == 0ull) {  // no row (or only NaN scores: the call fails)
            if (first) reinterpret_cast<unsigned long long*>(acc)[g] = MAXSIM_EMPTY_BITS;
            continue;
        }
        const double m = maxsim_score_dec(e);
        acc[g] = first ? m : acc[g] + m;
    }
}

int grid_for(uint64_t n, int per, int max_grid)
{
    const uint64_t blocks = (n + (uint64_t)per - 1) / (uint64_t)per;
    return (int)(blocks < 1 ? 1 : (blocks < (uint64_t)max_grid ? blocks : (uint64_t)max_grid));
}

template <int KSTEPS, int METRIC>
hipError_t launch_rows(hipStream_t s, dim3 grid, const void* slab, const float* nrm, const float* sqn, const void* q16, uint32_t nt,
                       uint32_t n_rows, const uint32_t* gor, uint32_t ng, uint32_t* M)
{
    hipLaunchKernelGGL((k_maxsim_rows<KSTEPS, METRIC>), grid, dim3(MS_NW * 64), 0, s, reinterpret_cast<const unsigned char*>(slab), nrm,
                       sqn, reinterpret_cast<const unsigned char*>(q16), nt, n_rows, gor, ng, M);
    return hipGetLastError();
}

template <int METRIC>
hipError_t launch_rows_ldb(hipStream_t s, uint32_t ldb, dim3 grid, const void* slab, const float* nrm, const float* sqn,
                           const void* q16, uint32_t nt, uint32_t n_rows, const uint32_t* gor, uint32_t ng, uint32_t* M)
{
    switch (ldb) {
    case 128: return launch_rows<8, METRIC>(s, grid, slab, nrm, sqn, q16, nt, n_rows, gor, ng, M);
    case 256: return launch_rows<16, METRIC>(s, grid, slab, nrm, sqn, q16, nt, n_rows, gor, ng, M);
    case 384: return launch_rows<24, METRIC>(s, grid, slab, nrm, sqn, q16, nt, n_rows, gor, ng, M);
    case 512: return launch_rows<32, METRIC>(s, grid, slab, nrm, sqn, q16, nt, n_rows, gor, ng, M);
    default: return launch_rows<48, METRIC>(s, grid, slab, nrm, sqn, q16, nt, n_rows, gor, ng, M);
    }
}

}  // namespace

bool maxsim_rows_supported(uint32_t dim, int metric)
{
    const uint32_t ldb = mfma_ldb(dim);
    if (metric != COSINE && metric != EUCLIDEAN && metric != DOT) return false;
    return dim >= 1 && (ldb == 128 || ldb == 256 || ldb == 384 || ldb == 512 || ldb == 768) && mfma_rows_kernel(dim);
}

hipError_t launch_maxsim_fill(hipStream_t s, uint32_t* p, uint64_t n, uint32_t v)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_maxsim_fill, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, p, (unsigned long long)n, v);
    return hipGetLastError();
}

hipError_t launch_maxsim_fill64(hipStream_t s, unsigned long long* p, uint64_t n, unsigned long long v)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_maxsim_fill64, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, p, (unsigned long long)n, v);
    return hipGetLastError();
}

hipError_t launch_maxsim_rows(hipStream_t s, int metric, const void* slab_frag, const float* row_norm, const float* row_sqnorm,
                              const void* q_bf16, uint32_t n_tokens, uint64_t n_rows, uint32_t dim, const uint32_t* group_of_row,
                              uint32_t n_groups, uint32_t* M, MaxsimRowsInfo* info)
{
    if (!maxsim_rows_supported(dim, metric) || n_rows == 0 || n_rows >= 0xFFFFFFE0ull || n_tokens == 0 ||
        n_tokens > MAXSIM_MAX_TOKENS || n_groups == 0 || !slab_frag || !q_bf16 || !group_of_row || !M)
        return hipErrorInvalidValue;
    if (metric != COSINE && (!row_norm || (metric == EUCLIDEAN && !row_sqnorm))) return hipErrorInvalidValue;
    const uint32_t ldb = mfma_ldb(dim);
    const uint32_t qpb = maxsim_qpb(ldb);
    const uint32_t chunks = (n_tokens + qpb - 1) / qpb;
    // one workgroup per CU (the tokens fill its LDS); at least one 32-row block per wave
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint64_t n_blocks = (n_rows + 31) / 32;
    const int gx = grid_for(n_blocks, MS_NW, cus > 0 ? cus : 256);
    if (info) {
        info->ksteps = (int)(ldb / 16);
        info->chunks = (int)chunks;
        info->grid_x = gx;
    }
    const dim3 grid(gx, chunks);
    switch (metric) {
    case COSINE:
        return launch_rows_ldb<COSINE>(s, ldb, grid, slab_frag, row_norm, row_sqnorm, q_bf16, n_tokens, (uint32_t)n_rows, group_of_row,
                                       n_groups, M);
    case EUCLIDEAN:
        return launch_rows_ldb<EUCLIDEAN>(s, ldb, grid, slab_frag, row_norm, row_sqnorm, q_bf16, n_tokens, (uint32_t)n_rows,
                                          group_of_row, n_groups, M);
    default:
        return launch_rows_ldb<DOT>(s, ldb, grid, slab_frag, row_norm, row_sqnorm, q_bf16, n_tokens, (uint32_t)n_rows, group_of_row,
                                    n_groups, M);
    }
}

hipError_t launch_maxsim_upper(hipStream_t s, int metric, const uint32_t* M, uint32_t n_tokens, uint32_t n_groups, uint32_t ldb,
                               double R, const double* q_norms, double* U, Cand64* lists, uint32_t* top, uint32_t* flag,
                               uint32_t* ctr)
{
    if (n_groups == 0 || n_tokens == 0 || n_tokens > MAXSIM_MAX_TOKENS) return hipErrorInvalidValue;
    const int grid = grid_for(n_groups, 1024, MAXSIM_TOP_LISTS);
    switch (metric) {
    case COSINE:
        hipLaunchKernelGGL(k_maxsim_upper<COSINE>, dim3(grid), dim3(1024), 0, s, M, n_tokens, n_groups, ldb, R, q_norms, U, lists, ctr);
        break;
    case EUCLIDEAN:
        hipLaunchKernelGGL(k_maxsim_upper<EUCLIDEAN>, dim3(grid), dim3(1024), 0, s, M, n_tokens, n_groups, ldb, R, q_norms, U, lists,
                           ctr);
        break;
    case DOT:
        hipLaunchKernelGGL(k_maxsim_upper<DOT>, dim3(grid), dim3(1024), 0, s, M, n_tokens, n_groups, ldb, R, q_norms, U, lists, ctr);
        break;
    default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_maxsim_top, dim3(1), dim3(1024), 0, s, (const Cand64*)lists, grid, top, flag, ctr);
    return hipGetLastError();
}

hipError_t launch_maxsim_survivors(hipStream_t s, const double* U, uint32_t n_groups, double L, uint32_t cap, uint32_t* list,
                                   uint32_t* flag, uint32_t* ctr)
{
    if (n_groups == 0 || cap == 0 || cap > MAXSIM_CAND_CAP) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_maxsim_survivors, dim3(grid_for(n_groups, 256, 2048)), dim3(256), 0, s, U, n_groups, L, cap, list, flag, ctr);
    return hipGetLastError();
}

hipError_t launch_maxsim_score(hipStream_t s, int metric, const double* master, const double* q64, uint32_t n_tokens, uint32_t dim,
                               const uint32_t* group_of_row, uint64_t n_rows, uint32_t n_groups, const uint32_t* flag,
                               const uint32_t* n_cand, uint32_t cap, MaxsimMember* members, uint32_t row_cap,
                               unsigned long long* E, double* scores, uint32_t* ctr)
{
    if (n_rows == 0 || n_rows >= 0xFFFFFFFFull || n_tokens == 0 || n_tokens > MAXSIM_MAX_TOKENS || cap == 0 ||
        cap > MAXSIM_CAND_CAP || row_cap == 0 || row_cap > MAXSIM_ROW_CAP)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_maxsim_members, dim3(grid_for(n_rows, 256, 4096)), dim3(256), 0, s, group_of_row, (uint32_t)n_rows, n_groups,
                       flag, members, row_cap, ctr);
    const int egrid = 4096;  // grid-stride over the device's own member count
    switch (metric) {
    case COSINE:
        hipLaunchKernelGGL(k_maxsim_exact<COSINE>, dim3(egrid), dim3(256), 0, s, master, q64, n_tokens, dim, (const MaxsimMember*)members,
                           row_cap, (uint32_t)n_rows, cap, E, ctr);
        break;
    case EUCLIDEAN:
        hipLaunchKernelGGL(k_maxsim_exact<EUCLIDEAN>, dim3(egrid), dim3(256), 0, s, master, q64, n_tokens, dim,
                           (const MaxsimMember*)members, row_cap, (uint32_t)n_rows, cap, E, ctr);
        break;
    case DOT:
        hipLaunchKernelGGL(k_maxsim_exact<DOT>, dim3(egrid), dim3(256), 0, s, master, q64, n_tokens, dim, (const MaxsimMember*)members,
                           row_cap, (uint32_t)n_rows, cap, E, ctr);
        break;
    default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_maxsim_sum, dim3(grid_for(cap, 256, 16)), dim3(256), 0, s, (const unsigned long long*)E, n_tokens, n_cand, cap,
                       scores);
    return hipGetLastError();
}

hipError_t launch_maxsim_rank(hipStream_t s, const uint32_t* list, const double* scores, const uint32_t* n_cand, uint32_t cap,
                              const unsigned long long* group_keys, uint32_t k, unsigned long long* out_keys, double* out_scores)
{
    if (cap == 0 || cap > MAXSIM_CAND_CAP || k == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_maxsim_rank, dim3(1), dim3(1024), 0, s, list, scores, n_cand, cap, group_keys, k, out_keys, out_scores);
    return hipGetLastError();
}

hipError_t launch_maxsim_token(hipStream_t s, const double* scores, const uint32_t* group_of_row, uint64_t n_rows,
                               uint32_t n_groups, bool first, unsigned long long* E1, double* acc, uint32_t* ctr)
{
    if (n_rows == 0 || n_rows >= 0xFFFFFFFFull || n_groups == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_maxsim_segmax, dim3(grid_for(n_rows, 256, 4096)), dim3(256), 0, s, scores, group_of_row, (uint32_t)n_rows,
                       n_groups, E1, ctr);
    hipLaunchKernelGGL(k_maxsim_acc, dim3(grid_for(n_groups, 256, 2048)), dim3(256), 0, s, E1, acc, n_groups, first ? 1u : 0u);
    return hipGetLastError();
}

}  // namespace vl
