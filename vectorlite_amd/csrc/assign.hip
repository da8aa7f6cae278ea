// assign.hip -- nearest-label assignment of every stored row: for each row, the best of up to 4096
// external label vectors under the reference score.
//
// k_assign_rows<KSTEPS, METRIC, MODE> is the hot kernel, on the matrix cores (v_mfma_f32_16x16x32_bf16).  It is the transpose
// of k_mfma_rows / k_maxsim_rows: ROWS STATIONARY, LABELS STREAMING.
//   A = a wave's own 32-row block of the fragment-major slab: 1 KB loads, the whole K in registers up to stride 384 (loaded
//       once per block, whatever the number of labels), four K phases at strides 512 and 768 (streamed again per label chunk).
//   B = the labels, in chunks of assign_chunk(stride) (64; 48 at stride 768) that the workgroup walks INSIDE the kernel through
//       two LDS buffers in k_mfma_rows' padded row layout (row stride + 32 bytes: conflict-free ds_read_b128).  A thread loads
//       its pieces of chunk c + 1 into registers in front of chunk c's MFMAs and writes them to the other buffer behind chunk
//       c's epilogue: the copy's latency hides under the MFMAs, and one barrier per chunk orders both buffers.  gridDim.y
//       carries no chunks: the slab is read from HBM once per pass.
//   C = a 32 x chunk tile per wave per chunk; the keys are assign_key (assign_plan.hpp), comparable across labels, formed
//       from the labels' scalars in LDS beside the chunk and the rows' norms in registers.
// MODE 0 (seed): per row the largest key and its label -- over the lane's accumulators in registers, across the 16 lanes
//   that hold a row's columns by four ds_bpermute steps -- carried across the chunks in 16 registers and stored once per row.
// MODE 1 (candidates): every label whose key reaches the row's threshold and that is not the row's seed goes to a per-wave
//   LDS ring, flushed with one returning atomic; the common path is a v_max3 tree per row, one compare each, one ballot.
//
// Behind it: k_assign_seed (the seed's reference score S and the row's threshold), k_assign_pairs / k_assign_resolve /
// k_assign_out (exact scores of the kept pairs, fetch-max, lowest label among the best, the winner's own bits), and
// k_assign_fold for the exact route.
#include "assign.hpp"

#include "device_common.hpp"
#include "mfma_scan.hpp"

namespace vl {

static_assert(ASSIGN_IN_EXTRA == IN_EXTRA_MFMA, "the assignment's sums are the batch filter's sums");
static_assert(COSINE == BOUND_COSINE && EUCLIDEAN == BOUND_EUCLIDEAN && DOT == BOUND_DOT, "metric codes");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {
using namespace dev;

constexpr int AS_NW = 8;     // waves per workgroup (two per SIMD)
constexpr int AS_SEG = 128;  // ring entries per wave: a flush whenever the next 64 might not fit

__device__ __forceinline__ float amax3(float a, float b, float c)
{
    return __builtin_fmaxf(__builtin_fmaxf(a, b), c);  // folds to v_max3_f32
}

template <int KSTEPS, int METRIC, int MODE>
__global__ __launch_bounds__(AS_NW * 64) void k_assign_rows(const unsigned char* __restrict__ slab, const float* __restrict__ row_nrm,
                                                            const unsigned char* __restrict__ q16, const float* __restrict__ lab_a,
                                                            const float* __restrict__ lab_b, uint32_t n_labels, uint32_t n_chunks,
                                                            uint32_t n_rows, uint32_t blk0, uint32_t blk1,
                                                            AssignSeed* __restrict__ seeds, const float* __restrict__ thr,
                                                            const uint32_t* __restrict__ seed_label, AssignCand* __restrict__ cand,
                                                            uint32_t* __restrict__ cnt, uint32_t cap)
{
    constexpr int LDB = KSTEPS * 16;
    constexpr int ROW_BYTES = LDB * 2;
    constexpr int LDS_ROW = ROW_BYTES + 32;
    constexpr int KS32 = KSTEPS / 2;               // K = 32 per MFMA
    constexpr int CH = (int)assign_chunk((uint32_t)LDB);
    constexpr int QB = CH / 16;                    // label blocks of a chunk
    constexpr int PH = KS32 > 12 ? 4 : 1;          // K phases: 16 = 4 x 4 (stride 512), 24 = 4 x 6 (stride 768)
    constexpr int KSP = KS32 / PH;                 // A fragments a wave holds per 16-row half block
    constexpr int GROUP_BYTES = 16 * ROW_BYTES;    // one 16-row group of the slab: KS32 chunks of 1 KB
    constexpr int BUF_BYTES = CH * LDS_ROW;
    constexpr int CPR = ROW_BYTES / 16;
    constexpr int NP = CH * CPR / (AS_NW * 64);    // 16-byte pieces of a chunk per thread
    constexpr int RING_BYTES = MODE == 1 ? AS_NW * AS_SEG * 8 : 0;
    // up to stride 256 a thread's pieces of the next chunk wait in registers across the MFMAs; beyond, the registers belong to
    // the A fragments and the copy goes straight through (the SIMD's other wave covers its latency)
    constexpr bool STAGED = LDB <= 256;
    static_assert(KS32 % PH == 0 && CH % 16 == 0 && (CH * CPR) % (AS_NW * 64) == 0 && 2 * CH <= AS_NW * 64, "whole phases and pieces");
    static_assert(2 * BUF_BYTES + 4 * CH * 4 + RING_BYTES <= 160 * 1024, "two label buffers, their scalars and the rings fit the LDS");

    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES + 4 * CH * 4 + RING_BYTES];
    float* scal = reinterpret_cast<float*>(lds + 2 * BUF_BYTES);  // [2][a: CH, b: CH]
    uint32_t* ring_row = reinterpret_cast<uint32_t*>(lds + 2 * BUF_BYTES + 4 * CH * 4);  // [NW][SEG] (MODE 1)
    uint32_t* ring_lab = ring_row + AS_NW * AS_SEG;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, kg = lane >> 4;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    const uint32_t row_base = blk0 * ASSIGN_BLOCK_ROWS;

    // ---- a chunk on its way to LDS: global -> registers in front of the MFMAs, registers -> LDS behind them ----
    u32x4 stage[NP];
    float stage_s = 0.f;
    auto stage_load = [&](uint32_t chunk) {
        const unsigned char* src = q16 + (size_t)chunk * CH * ROW_BYTES;
#pragma unroll
        for (int i = 0; i < NP; ++i) stage[i] = *reinterpret_cast<const u32x4*>(src + (size_t)(tid + i * AS_NW * 64) * 16);
        if (tid < 2 * CH) stage_s = tid < CH ? lab_a[chunk * CH + tid] : lab_b[chunk * CH + tid - CH];
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int c = tid + i * AS_NW * 64;
            *reinterpret_cast<u32x4*>(&lds[buf * BUF_BYTES + (c / CPR) * LDS_ROW + (c % CPR) * 16]) = stage[i];
        }
        if (tid < 2 * CH) scal[buf * 2 * CH + tid] = stage_s;
    };

    uint32_t my_cnt = 0;
    uint32_t* my_row = ring_row + wave * AS_SEG;
    uint32_t* my_lab = ring_lab + wave * AS_SEG;
    auto flush_wave = [&]() {  // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(cnt, my_cnt);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        for (uint32_t e = lane; e < my_cnt; e += 64) {
            const uint32_t slot = base + e;
            if (slot < cap) {  // a counter above cap tells the host that this range has to be split
                cand[slot].row = my_row[e];
                cand[slot].label = my_lab[e];
            }
        }
        my_cnt = 0;
    };
    auto append = [&](bool keep, uint32_t row, uint32_t label) {  // wave-uniform call
        const unsigned long long mk = __builtin_amdgcn_ballot_w64(keep);
        if (mk == 0ull) return;
        if (my_cnt + 64u > (uint32_t)AS_SEG) flush_wave();
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        if (keep) {
            my_row[my_cnt + rank] = row;
            my_lab[my_cnt + rank] = label;
        }
        my_cnt += (uint32_t)__popcll(mk);
    };

    stage_load(0);
    stage_store(0);
    __syncthreads();
    int buf = 0;
    const bool multi = n_chunks > 1;  // a single chunk stays in buffer 0: no copy and no barrier after this one

    // every wave of the workgroup makes the same number of rounds (the barriers); a wave without a block only copies
    const uint32_t per_round = gridDim.x * AS_NW;
    const uint32_t rounds = (blk1 - blk0 + per_round - 1) / per_round;
    auto a_ptr = [&](uint32_t blk) { return slab + (size_t)blk * (2 * GROUP_BYTES) + lane_off; };
    auto block_of = [&](uint32_t round) { return blk0 + (round * gridDim.x + blockIdx.x) * AS_NW + (uint32_t)wave; };
    bf16x8 afrag[2][KSP];
    {
        const uint32_t b = block_of(0);
        const unsigned char* p = a_ptr(b < blk1 ? b : blk1 - 1);
#pragma unroll
        for (int s = 0; s < KSP; ++s)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) afrag[rb][s] = *reinterpret_cast<const bf16x8*>(p + rb * GROUP_BYTES + s * 1024);
    }

    for (uint32_t round = 0; round < rounds; ++round) {
        const uint32_t b = block_of(round);
        const bool active = b < blk1;  // wave-uniform; once false it stays false
        const uint32_t bb = active ? b : blk1 - 1;
        const uint32_t nb = block_of(round + 1);
        const unsigned char* pc = a_ptr(bb);
        const unsigned char* pn = a_ptr(nb < blk1 ? nb : bb);
        const uint32_t row0 = bb * ASSIGN_BLOCK_ROWS;

        // this lane's rows 16 rb + 4 kg + jj: their scalars (row_nrm is allocated in whole 64-row tiles, the range's arrays in
        // whole blocks).  With the whole K in registers they are requested once per block, in front of the MFMAs; in the
        // phased shapes every register belongs to the fragments in flight and they are fetched per chunk behind the MFMAs
        f32x4 nrm[2] = {f32x4{1.f, 1.f, 1.f, 1.f}, f32x4{1.f, 1.f, 1.f, 1.f}};
        f32x4 th[2];
        u32x4 sd[2];
        auto load_scalars = [&]() {
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                if (METRIC != COSINE) nrm[rb] = *reinterpret_cast<const f32x4*>(row_nrm + row0 + 16 * rb + 4 * kg);
                if (MODE == 1) {
                    th[rb] = *reinterpret_cast<const f32x4*>(thr + (row0 - row_base) + 16 * rb + 4 * kg);
                    sd[rb] = *reinterpret_cast<const u32x4*>(seed_label + (row0 - row_base) + 16 * rb + 4 * kg);
                }
            }
        };
        if (PH == 1) load_scalars();
        float bk[2][4];
        uint32_t bl[2][4];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                bk[rb][jj] = -INFINITY;
                bl[rb][jj] = 0u;
            }

        for (uint32_t c = 0; c < n_chunks; ++c) {
            const bool last_chunk = c + 1 == n_chunks;
            const bool copy = multi && !(last_chunk && round + 1 == rounds);  // workgroup-uniform
            if (copy) {
                stage_load(last_chunk ? 0u : c + 1);
                if (!STAGED) stage_store(buf ^ 1);
            }
            if (active) {
                const unsigned char* qrow = &lds[buf * BUF_BYTES + c16 * LDS_ROW + kg * 16];
                f32x4 acc[2][QB];
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int j = 0; j < QB; ++j) acc[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ph = 0; ph < PH; ++ph) {
                    // the fragments are refilled behind their last use: with the block's next K phase; after the last phase with
                    // its first one again for the next chunk, or with the wave's next block after the last chunk
                    const unsigned char* psrc = ph + 1 < PH ? pc + (size_t)(ph + 1) * KSP * 1024 : (last_chunk ? pn : pc);
                    const bool refill = PH > 1 || last_chunk;  // wave-uniform
#pragma unroll
                    for (int s = 0; s < KSP; ++s) {
                        const unsigned char* bp = qrow + (ph * KSP + s) * 64;
#pragma unroll
                        for (int j = 0; j < QB; ++j) {
                            const bf16x8 bq = *reinterpret_cast<const bf16x8*>(bp + j * 16 * LDS_ROW);
                            acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[0][s], bq, acc[0][j], 0, 0, 0);
                            acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[1][s], bq, acc[1][j], 0, 0, 0);
                        }
                        if (refill) {
#pragma unroll
                            for (int rb = 0; rb < 2; ++rb)
                                afrag[rb][s] = *reinterpret_cast<const bf16x8*>(psrc + rb * GROUP_BYTES + s * 1024);
                        }
                    }
                }

                if (PH > 1) load_scalars();
                // ---- epilogue: C layout of a 16x16 block: column = lane & 15 (label), row = 4 (lane >> 4) + reg ----
                const float* sa = scal + buf * 2 * CH + c16;
                const float* sb = sa + CH;
                auto key_of = [&](int rb, int j, int jj) -> float {
                    return assign_key<METRIC>(acc[rb][j][jj], nrm[rb][jj], METRIC == COSINE ? sa[16 * j] : 1.0f, sb[16 * j]);
                };
                if constexpr (MODE == 0) {
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            float m = key_of(rb, 0, jj);
                            uint32_t l = (uint32_t)c16;
#pragma unroll
                            for (int j = 1; j < QB; ++j) {
                                const float k = key_of(rb, j, jj);
                                if (k > m) {
                                    m = k;
                                    l = (uint32_t)(16 * j + c16);
                                }
                            }
#pragma unroll
                            for (int off = 1; off < 16; off <<= 1) {  // the 16 lanes of one kg hold the row's other columns
                                const float om = __shfl_xor(m, off);
                                const uint32_t ol = (uint32_t)__shfl_xor((int)l, off);
                                if (om > m || (om == m && ol < l)) {
                                    m = om;
                                    l = ol;
                                }
                            }
                            if (m > bk[rb][jj]) {  // an earlier chunk keeps a tie
                                bk[rb][jj] = m;
                                bl[rb][jj] = c * (uint32_t)CH + l;
                            }
                        }
                } else {
                    bool hit = false;
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            float m = key_of(rb, 0, jj);
#pragma unroll
                            for (int j = 1; j + 1 < QB; j += 2) m = amax3(m, key_of(rb, j, jj), key_of(rb, j + 1, jj));
                            if (QB % 2 == 0) m = fmaxf(m, key_of(rb, QB - 1, jj));
                            hit |= m >= th[rb][jj];
                        }
                    if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
                        // at least the seeds' own chunks come here; only THIS wave pays for it
#pragma unroll
                        for (int j = 0; j < QB; ++j) {
                            const uint32_t label = c * (uint32_t)CH + (uint32_t)(16 * j + c16);
#pragma unroll
                            for (int rb = 0; rb < 2; ++rb) {
                                bool in[4];
#pragma unroll
                                for (int jj = 0; jj < 4; ++jj) in[jj] = key_of(rb, j, jj) >= th[rb][jj];
                                if (__builtin_amdgcn_ballot_w64(in[0] || in[1] || in[2] || in[3]) == 0ull) continue;  // wave-uniform
#pragma unroll
                                for (int jj = 0; jj < 4; ++jj) {
                                    const uint32_t row = row0 + (uint32_t)(16 * rb + 4 * kg + jj);
                                    append(in[jj] && row < n_rows && label < n_labels && label != sd[rb][jj], row, label);
                                }
                            }
                        }
                    }
                }
            }
            if (multi) {
                if (copy && STAGED) stage_store(buf ^ 1);
                __syncthreads();  // the other buffer is written, this one consumed
                buf ^= 1;
            }
        }

        if (MODE == 0 && active && c16 == 0) {  // one plain 8-byte store per row
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const uint32_t row = row0 + (uint32_t)(16 * rb + 4 * kg + jj);
                    if (row < n_rows) seeds[row - row_base] = AssignSeed{bk[rb][jj], bl[rb][jj]};
                }
        }
    }
    if (MODE == 1 && my_cnt) flush_wave();
}

// the labels' scalars; one thread per (padded) label
template <int METRIC>
__global__ __launch_bounds__(256) void k_assign_labels(const double* __restrict__ norms, uint32_t n_labels, uint32_t n_pad, uint32_t ldb,
                                                       double R, float* __restrict__ a, float* __restrict__ b_seed,
                                                       float* __restrict__ b_keep)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_pad) return;
    AssignLabel l{0.f, -INFINITY, -INFINITY};  // a padding label: no row keeps it
    if (c < n_labels) l = assign_label<METRIC>(ldb, R, norms[c]);
    a[c] = l.a;
    b_seed[c] = l.b_seed;
    b_keep[c] = l.b_keep;
}

template <int METRIC>
__device__ __forceinline__ double exact_score(const double* __restrict__ x, const double* __restrict__ y, uint32_t dim)
{
    Acc64<METRIC> A;
    A.init();
    for (uint32_t c = 0; c < dim; ++c) A.step(x[c], y[c]);
    return A.score();
}

// One thread per row of the range: S = the reference score of (row, seed), Acc64 in index order, and what the second pass
// and the tail start from.
template <int METRIC>
__global__ __launch_bounds__(256) void k_assign_seed(const double* __restrict__ master, const double* __restrict__ labels64,
                                                     const float* __restrict__ row_sqn, uint32_t n_labels, uint32_t n_rows, uint32_t dim,
                                                     uint32_t ldb, uint32_t row_base, uint32_t range_rows, AssignRows rows,
                                                     uint32_t* __restrict__ ctr)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= range_rows) return;
    const uint32_t row = row_base + i;
    rows.winner[i] = 0xFFFFFFFFu;
    if (row >= n_rows) {  // the padding of the last block: no key reaches +inf
        rows.thr[i] = INFINITY;
        rows.seed_label[i] = 0u;
        rows.best[i] = 0ull;
        return;
    }
    uint32_t l = rows.seeds[i].label;
    if (l >= n_labels) l = 0u;
    const double S = exact_score<METRIC>(master + (size_t)row * dim, labels64 + (size_t)l * dim, dim);
    if (S != S) ctr[ASSIGN_CTR_NAN] = 1u;
    rows.S[i] = S;
    rows.seed_label[i] = l;
    rows.best[i] = S != S ? 0ull : assign_score_enc(S);
    rows.thr[i] = assign_row_threshold<METRIC>(ldb, S, METRIC == EUCLIDEAN ? row_sqn[row] : 0.f);
}

// the exact score of every kept pair; fetch-max into the row's best
template <int METRIC>
__global__ __launch_bounds__(256) void k_assign_pairs(AssignCand* __restrict__ cand, uint32_t cap, const double* __restrict__ master,
                                                      const double* __restrict__ labels64, uint32_t n_labels, uint32_t n_rows,
                                                      uint32_t dim, uint32_t row_base, uint32_t range_rows,
                                                      unsigned long long* __restrict__ best, uint32_t* __restrict__ ctr)
{
    const uint32_t m = ctr[ASSIGN_CTR_CAND];
    if (m > cap) return;  // the buffer is incomplete: the host splits the range
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < m; e += gridDim.x * 256) {
        const uint32_t row = cand[e].row, l = cand[e].label;
        if (row >= n_rows || row - row_base >= range_rows || l >= n_labels) continue;
        const double sc = exact_score<METRIC>(master + (size_t)row * dim, labels64 + (size_t)l * dim, dim);
        cand[e].score = sc;
        if (sc != sc) ctr[ASSIGN_CTR_NAN] = 1u;
        else atomicMax(best + (row - row_base), assign_score_enc(sc));
    }
}

__device__ __forceinline__ uint32_t winner_word(uint32_t label, double score)
{
    return (label << 1) | ((unsigned long long)__double_as_longlong(score) == 0x8000000000000000ull ? 1u : 0u);
}

// the lowest label among the seed and the pairs that reach the row's best
__global__ __launch_bounds__(256) void k_assign_resolve(const AssignCand* __restrict__ cand, uint32_t cap, uint32_t n_labels,
                                                        uint32_t n_rows, uint32_t row_base, uint32_t range_rows, AssignRows rows,
                                                        const uint32_t* __restrict__ ctr)
{
    const uint32_t m = ctr[ASSIGN_CTR_CAND];
    if (m > cap) return;
    const uint32_t total = m > range_rows ? m : range_rows;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        if (e < range_rows && row_base + e < n_rows) {
            const double S = rows.S[e];
            if (S == S && assign_score_enc(S) == rows.best[e]) atomicMin(rows.winner + e, winner_word(rows.seed_label[e], S));
        }
        if (e < m) {
            const uint32_t row = cand[e].row, l = cand[e].label;
            if (row >= n_rows || row - row_base >= range_rows || l >= n_labels) continue;
            const double sc = cand[e].score;
            if (sc == sc && assign_score_enc(sc) == rows.best[row - row_base]) atomicMin(rows.winner + (row - row_base), winner_word(l, sc));
        }
    }
}

// the winner's label and its own score bits (the encoding folds -0.0 onto +0.0; the winner's word kept the sign)
__global__ __launch_bounds__(256) void k_assign_out(uint32_t cap, uint32_t range_rows, AssignRows rows, const uint32_t* __restrict__ ctr)
{
    if (ctr[ASSIGN_CTR_CAND] > cap) return;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= range_rows) return;
    const uint32_t w = rows.winner[i];
    const double s = assign_score_dec(rows.best[i]);
    rows.out_labels[i] = (unsigned long long)(w >> 1);
    rows.out_scores[i] = (w & 1u) ? -0.0 : s;
}

__global__ __launch_bounds__(256) void k_assign_fold(const double* __restrict__ scores, uint32_t n_rows, uint32_t l,
                                                     double* __restrict__ best, uint32_t* __restrict__ label, uint32_t* __restrict__ ctr)
{
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < n_rows; p += gridDim.x * 256) {
        const double sc = scores[p];
        if (sc != sc) {
            ctr[ASSIGN_CTR_NAN] = 1u;
            continue;
        }
        if (l == 0 || assign_score_enc(sc) > assign_score_enc(best[p])) {
            best[p] = sc;
            label[p] = l;
        }
    }
}

int grid_for(uint64_t n, int per, int max_grid)
{
    const uint64_t blocks = (n + (uint64_t)per - 1) / (uint64_t)per;
    return (int)(blocks < 1 ? 1 : (blocks < (uint64_t)max_grid ? blocks : (uint64_t)max_grid));
}

struct RowsArgs {
    const void *slab, *q16;
    const float *row_nrm, *a, *b;
    uint32_t n_labels, n_chunks, n_rows;
    AssignRange r;
    AssignRows rows;
    AssignCand* cand;
    uint32_t* cnt;
    uint32_t cap, grid;
};

template <int KSTEPS, int METRIC, int MODE>
hipError_t launch_rows(hipStream_t s, const RowsArgs& x)
{
    hipLaunchKernelGGL((k_assign_rows<KSTEPS, METRIC, MODE>), dim3(x.grid), dim3(AS_NW * 64), 0, s,
                       reinterpret_cast<const unsigned char*>(x.slab), x.row_nrm, reinterpret_cast<const unsigned char*>(x.q16), x.a, x.b,
                       x.n_labels, x.n_chunks, x.n_rows, x.r.b0, x.r.b1, x.rows.seeds, x.rows.thr, x.rows.seed_label, x.cand, x.cnt,
                       x.cap);
    return hipGetLastError();
}

template <int METRIC, int MODE>
hipError_t launch_rows_ldb(hipStream_t s, uint32_t ldb, const RowsArgs& x)
{
    switch (ldb) {
    case 128: return launch_rows<8, METRIC, MODE>(s, x);
    case 256: return launch_rows<16, METRIC, MODE>(s, x);
    case 384: return launch_rows<24, METRIC, MODE>(s, x);
    case 512: return launch_rows<32, METRIC, MODE>(s, x);
    default: return launch_rows<48, METRIC, MODE>(s, x);
    }
}

template <int METRIC>
hipError_t launch_rows_mode(hipStream_t s, int mode, uint32_t ldb, const RowsArgs& x)
{
    return mode == 0 ? launch_rows_ldb<METRIC, 0>(s, ldb, x) : launch_rows_ldb<METRIC, 1>(s, ldb, x);
}

bool range_ok(AssignRange r, uint64_t n_rows)
{
    return r.b0 < r.b1 && (uint64_t)r.b1 <= (n_rows + ASSIGN_BLOCK_ROWS - 1) / ASSIGN_BLOCK_ROWS;
}

}  // namespace

bool assign_rows_supported(uint32_t dim, int metric)
{
    const uint32_t ldb = mfma_ldb(dim);
    if (metric != COSINE && metric != EUCLIDEAN && metric != DOT) return false;
    return dim >= 1 && (ldb == 128 || ldb == 256 || ldb == 384 || ldb == 512 || ldb == 768) && mfma_rows_kernel(dim);
}

hipError_t launch_assign_labels(hipStream_t s, int metric, const double* label_norms, uint32_t n_labels, uint32_t n_pad, uint32_t ldb,
                                double R, float* a, float* b_seed, float* b_keep)
{
    if (n_labels == 0 || n_labels > ASSIGN_MAX_LABELS || n_pad < n_labels) return hipErrorInvalidValue;
    const dim3 grid((n_pad + 255) / 256);
    switch (metric) {
    case COSINE: hipLaunchKernelGGL(k_assign_labels<COSINE>, grid, dim3(256), 0, s, label_norms, n_labels, n_pad, ldb, R, a, b_seed, b_keep); break;
    case EUCLIDEAN:
        hipLaunchKernelGGL(k_assign_labels<EUCLIDEAN>, grid, dim3(256), 0, s, label_norms, n_labels, n_pad, ldb, R, a, b_seed, b_keep);
        break;
    case DOT: hipLaunchKernelGGL(k_assign_labels<DOT>, grid, dim3(256), 0, s, label_norms, n_labels, n_pad, ldb, R, a, b_seed, b_keep); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_assign_rows(hipStream_t s, int metric, int mode, const void* slab_frag, const float* row_norm, const void* q_bf16,
                              const float* a, const float* b, uint32_t n_labels, uint64_t n_rows, uint32_t dim, AssignRange r,
                              const AssignRows& rows, AssignCand* cand, uint32_t cap, uint32_t* ctr)
{
    if (!assign_rows_supported(dim, metric) || n_rows == 0 || n_rows >= 0xFFFFFFE0ull || n_labels == 0 || n_labels > ASSIGN_MAX_LABELS ||
        !range_ok(r, n_rows) || !slab_frag || !q_bf16 || !a || !b || (mode != 0 && mode != 1))
        return hipErrorInvalidValue;
    if (metric != COSINE && !row_norm) return hipErrorInvalidValue;
    if (mode == 0 ? !rows.seeds : (!rows.thr || !rows.seed_label || !cand || !ctr || cap == 0)) return hipErrorInvalidValue;
    const uint32_t ldb = mfma_ldb(dim);
    const uint32_t ch = assign_chunk(ldb);
    // one workgroup per CU (the label buffers fill its LDS); at least one 32-row block per wave
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const RowsArgs x{slab_frag, q_bf16, row_norm, a, b, n_labels, (n_labels + ch - 1) / ch, (uint32_t)n_rows, r, rows, cand,
                     ctr ? ctr + ASSIGN_CTR_CAND : nullptr, cap, (uint32_t)grid_for(r.b1 - r.b0, AS_NW, cus > 0 ? cus : 256)};
    switch (metric) {
    case COSINE: return launch_rows_mode<COSINE>(s, mode, ldb, x);
    case EUCLIDEAN: return launch_rows_mode<EUCLIDEAN>(s, mode, ldb, x);
    default: return launch_rows_mode<DOT>(s, mode, ldb, x);
    }
}

hipError_t launch_assign_seed(hipStream_t s, int metric, const double* master, const double* labels64, const float* row_sqnorm,
                              uint32_t n_labels, uint64_t n_rows, uint32_t dim, AssignRange r, const AssignRows& rows, uint32_t* ctr)
{
    if (!range_ok(r, n_rows) || n_rows >= 0xFFFFFFE0ull || n_labels == 0 || (metric == EUCLIDEAN && !row_sqnorm)) return hipErrorInvalidValue;
    const uint32_t range_rows = (r.b1 - r.b0) * ASSIGN_BLOCK_ROWS, row_base = r.b0 * ASSIGN_BLOCK_ROWS, ldb = mfma_ldb(dim);
    const dim3 grid((range_rows + 255) / 256);
#define VL_ASSIGN_SEED(M)                                                                                                       \
    hipLaunchKernelGGL(k_assign_seed<M>, grid, dim3(256), 0, s, master, labels64, row_sqnorm, n_labels, (uint32_t)n_rows, dim, ldb, \
                       row_base, range_rows, rows, ctr)
    switch (metric) {
    case COSINE: VL_ASSIGN_SEED(COSINE); break;
    case EUCLIDEAN: VL_ASSIGN_SEED(EUCLIDEAN); break;
    case DOT: VL_ASSIGN_SEED(DOT); break;
    default: return hipErrorInvalidValue;
    }
#undef VL_ASSIGN_SEED
    return hipGetLastError();
}

hipError_t launch_assign_finish(hipStream_t s, int metric, const double* master, const double* labels64, uint32_t n_labels,
                                uint64_t n_rows, uint32_t dim, AssignRange r, const AssignRows& rows, AssignCand* cand, uint32_t cap,
                                uint32_t* ctr)
{
    if (!range_ok(r, n_rows) || n_rows >= 0xFFFFFFE0ull || n_labels == 0 || cap == 0) return hipErrorInvalidValue;
    const uint32_t range_rows = (r.b1 - r.b0) * ASSIGN_BLOCK_ROWS, row_base = r.b0 * ASSIGN_BLOCK_ROWS;
    const dim3 pgrid(4096);  // grid-stride over the device's own pair count
#define VL_ASSIGN_PAIRS(M)                                                                                                         \
    hipLaunchKernelGGL(k_assign_pairs<M>, pgrid, dim3(256), 0, s, cand, cap, master, labels64, n_labels, (uint32_t)n_rows, dim, row_base, \
                       range_rows, rows.best, ctr)
    switch (metric) {
    case COSINE: VL_ASSIGN_PAIRS(COSINE); break;
    case EUCLIDEAN: VL_ASSIGN_PAIRS(EUCLIDEAN); break;
    case DOT: VL_ASSIGN_PAIRS(DOT); break;
    default: return hipErrorInvalidValue;
    }
#undef VL_ASSIGN_PAIRS
    hipLaunchKernelGGL(k_assign_resolve, pgrid, dim3(256), 0, s, (const AssignCand*)cand, cap, n_labels, (uint32_t)n_rows, row_base,
                       range_rows, rows, (const uint32_t*)ctr);
    hipLaunchKernelGGL(k_assign_out, dim3((range_rows + 255) / 256), dim3(256), 0, s, cap, range_rows, rows, (const uint32_t*)ctr);
    return hipGetLastError();
}

hipError_t launch_assign_fold(hipStream_t s, const double* scores, uint64_t n_rows, uint32_t l, double* best, uint32_t* label,
                              uint32_t* ctr)
{
    if (n_rows == 0 || n_rows >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_assign_fold, dim3(grid_for(n_rows, 256, 4096)), dim3(256), 0, s, scores, (uint32_t)n_rows, l, best, label, ctr);
    return hipGetLastError();
}

}  // namespace vl
