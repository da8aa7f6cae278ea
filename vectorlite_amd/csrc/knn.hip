// knn.hip -- the exact k-nearest-neighbour graph of the stored rows: for every row its k best other
// rows under the reference score.
//
// k_knn_rows<KSTEPS, METRIC, MODE> is the hot kernel, on the matrix cores (v_mfma_f32_16x16x32_bf16): ROWS STATIONARY,
// COLUMNS STREAMING over the full square, both operands blocks of the index's own fragment-major slab.
//   A = a wave's own 32-row block, as k_assign_rows keeps it: the whole K in registers up to stride 384 (loaded once per
//       block), four K phases at strides 512 and 768.
//   B = the slab's own rows in chunks of knn_chunk(stride) (64; 48 at stride 768) that the workgroup walks INSIDE the kernel.
//       A chunk is one contiguous byte range of the slab, copied with 16-byte pieces and read back with ds_read_b128 at
//       lane * 16: for the 16x16x32 shape a 1 KB slab chunk IS a B fragment (section 29), so there is no re-layout and no
//       padding.  Two buffers up to stride 256 (the next chunk's copy runs under this chunk's MFMAs, one barrier per chunk);
//       one buffer beyond, where the lists need the LDS (two barriers per chunk).  16-row groups past the last row are zeros.
//   C = a 32 x chunk tile per wave per chunk.  Keys are the join's: the cosine sum, or join_pair_key of the sum and the two
//       rows' norm16 (Euclidean, dot) -- comparable across columns for one row.
// MODE 0 (seeds): per-row top-k state carried across the stream.  Each row owns k (key, position) entries in LDS (entry-major:
//   32 rows side by side, 8 KB per wave) and a running threshold -- its k-th key, -inf while the list is short -- that the
//   lanes holding the row keep in registers.  Insertion is lazy: a v_max3 tree per row over the tile, one compare each, one
//   ballot, one branch; behind it the keys above their own row's threshold go to the wave's LDS ring, and the ring is folded
//   into the lists (lane r owns row r: replace the smallest entry, one scan) when the next 64 entries might not fit.
//   The self pair and columns past the last row never enter.  Ties fall anywhere: seeds only have to be k distinct partners.
// MODE 1 (keep): every (row, column != row) whose key reaches the row's threshold goes through the ring to the range's
//   candidate buffer, one returning atomic per flush.
//
// Behind it: k_knn_seed (the seeds' reference scores, S = the k-th largest, the join's threshold for min_score = S),
// k_knn_pairs (the kept pairs' reference scores), the sort of all records by (row, score desc, partner) on kernels.hip's
// bitonic network, and k_knn_emit (per row the first kk distinct partners).
#include "knn.hpp"

#include "device_common.hpp"
#include "join_plan.hpp"
#include "mfma_scan.hpp"

namespace vl {

static_assert(JOIN_IN_EXTRA == IN_EXTRA_MFMA, "the graph's keys are the batch filter's keys");
static_assert(COSINE == BOUND_COSINE && EUCLIDEAN == BOUND_EUCLIDEAN && DOT == BOUND_DOT, "metric codes");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {
using namespace dev;

constexpr int KN_NW = 8;     // waves per workgroup (two per SIMD)
constexpr int KN_SEG = 128;  // ring entries per wave: folded or flushed whenever the next 64 might not fit
constexpr int KN_K = (int)KNN_MAX_K;

__device__ __forceinline__ float kmax3(float a, float b, float c)
{
    return __builtin_fmaxf(__builtin_fmaxf(a, b), c);  // folds to v_max3_f32
}

template <int KSTEPS, int METRIC, int MODE>
__global__ __launch_bounds__(KN_NW * 64) void k_knn_rows(const unsigned char* __restrict__ slab, const float* __restrict__ row_nrm,
                                                         uint32_t n_rows, uint32_t n_chunks, uint32_t blk0, uint32_t blk1, uint32_t k,
                                                         float e32, uint32_t* __restrict__ seeds, const float* __restrict__ thr,
                                                         KnnCand* __restrict__ cand, uint32_t* __restrict__ cnt, uint32_t cap)
{
    constexpr int LDB = KSTEPS * 16;
    constexpr int ROW_BYTES = LDB * 2;
    constexpr int KS32 = KSTEPS / 2;             // K = 32 per MFMA
    constexpr int CH = (int)knn_chunk((uint32_t)LDB);
    constexpr int QB = CH / 16;                  // 16-row groups of a chunk
    constexpr int PH = KS32 > 12 ? 4 : 1;        // K phases: 16 = 4 x 4 (stride 512), 24 = 4 x 6 (stride 768)
    constexpr int KSP = KS32 / PH;               // A fragments a wave holds per 16-row half block
    constexpr int GROUP_BYTES = 16 * ROW_BYTES;  // one 16-row group of the slab: KS32 chunks of 1 KB
    constexpr int BUF_BYTES = CH * ROW_BYTES;
    constexpr int NBUF = LDB <= 256 ? 2 : 1;
    constexpr bool PAIR = METRIC != COSINE;      // per-pair scalars in the epilogue
    constexpr int PIECES = BUF_BYTES / 16;
    constexpr int GROUP_PIECES = GROUP_BYTES / 16;
    constexpr int COLN_BYTES = NBUF * CH * 4;
    constexpr int RING_BYTES = KN_NW * KN_SEG * (MODE == 0 ? 12 : 8);
    constexpr int LIST_BYTES = MODE == 0 ? KN_NW * (2 * KN_K * 32 * 4 + 32 * 4) : 0;
    static_assert(KS32 % PH == 0 && CH % 16 == 0, "whole K phases; chunks are whole 16-row groups");
    static_assert(NBUF * BUF_BYTES + COLN_BYTES + RING_BYTES + LIST_BYTES <= 160 * 1024, "column buffers, rings and lists fit the LDS");

    __shared__ __attribute__((aligned(16))) unsigned char lds[NBUF * BUF_BYTES + COLN_BYTES + RING_BYTES + LIST_BYTES];
    float* col_n = reinterpret_cast<float*>(lds + NBUF * BUF_BYTES);                  // [NBUF][CH] the chunk rows' norm16 (PAIR)
    uint32_t* ring_a = reinterpret_cast<uint32_t*>(lds + NBUF * BUF_BYTES + COLN_BYTES);  // [NW][SEG] row (mode 0: within the block)
    uint32_t* ring_b = ring_a + KN_NW * KN_SEG;                                        // column
    float* ring_key = reinterpret_cast<float*>(ring_b + KN_NW * KN_SEG);               // (mode 0)
    float* list_key = reinterpret_cast<float*>(lds + NBUF * BUF_BYTES + COLN_BYTES + RING_BYTES);  // [NW][K][32] (mode 0)
    uint32_t* list_pos = reinterpret_cast<uint32_t*>(list_key + KN_NW * KN_K * 32);
    float* list_thr = reinterpret_cast<float*>(list_pos + KN_NW * KN_K * 32);          // [NW][32]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, kg = lane >> 4;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    const uint32_t row_base = blk0 * KNN_BLOCK_ROWS;
    const uint32_t n_groups = (n_rows + 15u) / 16u;  // 16-row groups that hold a row

    // ---- a chunk -> LDS as it lies in the slab ----
    auto copy_chunk = [&](uint32_t chunk, int buf) {
        const uint32_t col0 = chunk * (uint32_t)CH;
        const unsigned char* src = slab + (size_t)col0 * ROW_BYTES;
        const uint32_t g0 = col0 / 16u;
        for (int c = tid; c < PIECES; c += KN_NW * 64) {
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (g0 + (uint32_t)(c / GROUP_PIECES) < n_groups) v = *reinterpret_cast<const u32x4*>(src + (size_t)c * 16);
            *reinterpret_cast<u32x4*>(&lds[buf * BUF_BYTES + c * 16]) = v;
        }
        if (PAIR && tid < CH) {
            const uint32_t pos = col0 + (uint32_t)tid;
            col_n[buf * CH + tid] = pos < n_rows ? row_nrm[pos] : 0.f;
        }
    };

    uint32_t my_cnt = 0;  // wave-uniform
    uint32_t* my_a = ring_a + wave * KN_SEG;
    uint32_t* my_b = ring_b + wave * KN_SEG;
    float* my_key = ring_key + wave * KN_SEG;
    float* my_lkey = list_key + wave * KN_K * 32;
    uint32_t* my_lpos = list_pos + wave * KN_K * 32;
    float* my_lthr = list_thr + wave * 32;

    // mode 0: lane r < 32 owns row r of the wave's block -- the length of its list and its smallest key
    uint32_t l_cnt = 0;
    float l_min = -INFINITY;
    float th[2][4];  // this lane's rows 16 rb + 4 kg + jj: the running threshold (mode 0), the row's threshold (mode 1)
    uint32_t row0 = 0;

    auto fold = [&]() {  // mode 0, wave-uniform: the ring into the lists, then every lane's thresholds again
        __builtin_amdgcn_wave_barrier();
        if (lane < 32) {
            for (uint32_t e = 0; e < my_cnt; ++e) {
                if (my_a[e] != (uint32_t)lane) continue;
                const float key = my_key[e];
                const uint32_t pos = my_b[e];
                if (l_cnt < k) {
                    my_lkey[l_cnt * 32 + lane] = key;
                    my_lpos[l_cnt * 32 + lane] = pos;
                    l_min = l_cnt == 0 ? key : fminf(l_min, key);
                    ++l_cnt;
                } else if (key > l_min) {  // replaces the smallest entry; the new smallest is the old second or the key
                    uint32_t at = 0;
                    float m1 = my_lkey[lane], m2 = INFINITY;
                    for (uint32_t i = 1; i < k; ++i) {
                        const float v = my_lkey[i * 32 + lane];
                        if (v < m1) {
                            m2 = m1;
                            m1 = v;
                            at = i;
                        } else if (v < m2) {
                            m2 = v;
                        }
                    }
                    my_lkey[at * 32 + lane] = key;
                    my_lpos[at * 32 + lane] = pos;
                    l_min = fminf(m2, key);
                }
            }
            my_lthr[lane] = l_cnt == k ? l_min : -INFINITY;
        }
        my_cnt = 0;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int r = 16 * rb + 4 * kg + jj;
                th[rb][jj] = row0 + (uint32_t)r < n_rows ? my_lthr[r] : INFINITY;
            }
    };
    auto flush_wave = [&]() {  // mode 1, wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(cnt, my_cnt);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        for (uint32_t e = lane; e < my_cnt; e += 64) {
            const uint32_t slot = base + e;
            if (slot < cap) cand[slot] = KnnCand{my_a[e], my_b[e]};  // a counter above cap: the host splits the range
        }
        my_cnt = 0;
    };
    auto append = [&](bool keep, uint32_t row, uint32_t col, float key) {  // wave-uniform call
        const unsigned long long mk = __builtin_amdgcn_ballot_w64(keep);
        if (mk == 0ull) return;
        if (my_cnt + 64u > (uint32_t)KN_SEG) {
            if (MODE == 0) fold();
            else flush_wave();
        }
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        if (keep) {
            my_a[my_cnt + rank] = row;
            my_b[my_cnt + rank] = col;
            if (MODE == 0) my_key[my_cnt + rank] = key;
        }
        my_cnt += (uint32_t)__popcll(mk);
    };

    copy_chunk(0, 0);
    __syncthreads();
    int buf = 0;

    // every wave of the workgroup makes the same number of rounds (the barriers); a wave without a block only copies
    const uint32_t per_round = gridDim.x * KN_NW;
    const uint32_t rounds = (blk1 - blk0 + per_round - 1) / per_round;
    auto a_ptr = [&](uint32_t blk) { return slab + (size_t)blk * (2 * GROUP_BYTES) + lane_off; };
    auto block_of = [&](uint32_t round) { return blk0 + (round * gridDim.x + blockIdx.x) * KN_NW + (uint32_t)wave; };
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
        row0 = bb * KNN_BLOCK_ROWS;

        // this lane's rows 16 rb + 4 kg + jj: their norms (row_nrm is allocated in whole 64-row tiles) and, in mode 1, their
        // thresholds (the range's array holds whole blocks).  In the phased shapes the registers belong to the fragments in
        // flight and the norms are fetched per chunk behind the MFMAs.
        f32x4 nrm[2] = {f32x4{1.f, 1.f, 1.f, 1.f}, f32x4{1.f, 1.f, 1.f, 1.f}};
        auto load_norms = [&]() {
            if (PAIR) {
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) nrm[rb] = *reinterpret_cast<const f32x4*>(row_nrm + row0 + 16 * rb + 4 * kg);
            }
        };
        if (PH == 1) load_norms();
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const uint32_t r = row0 + (uint32_t)(16 * rb + 4 * kg + jj);
                if (MODE == 0) th[rb][jj] = r < n_rows ? -INFINITY : INFINITY;
                else th[rb][jj] = thr[r - row_base];
            }
        l_cnt = 0;
        l_min = -INFINITY;

        for (uint32_t c = 0; c < n_chunks; ++c) {
            const bool last_chunk = c + 1 == n_chunks;
            if (NBUF == 2) {
                if (!(last_chunk && round + 1 == rounds)) copy_chunk(last_chunk ? 0u : c + 1, buf ^ 1);  // workgroup-uniform
            } else if (c != 0 || round != 0) {
                __syncthreads();  // the previous chunk is consumed
                copy_chunk(c, 0);
                __syncthreads();
            }
            if (active) {
                const unsigned char* panel = &lds[buf * BUF_BYTES];
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
                        const unsigned char* bp = panel + (size_t)(ph * KSP + s) * 1024 + lane_off;
#pragma unroll
                        for (int j = 0; j < QB; ++j) {
                            const bf16x8 bq = *reinterpret_cast<const bf16x8*>(bp + (size_t)j * GROUP_BYTES);
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

                if (PH > 1) load_norms();
                // ---- epilogue: C layout of a 16x16 block: column = lane & 15 (chunk row), row = 4 (lane >> 4) + reg ----
                const float* cn = col_n + buf * CH + c16;
                auto key_of = [&](int rb, int j, int jj) -> float {
                    return join_pair_key<METRIC>(acc[rb][j][jj], e32, nrm[rb][jj], PAIR ? cn[16 * j] : 1.0f);
                };
                bool hit = false;
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        float m = key_of(rb, 0, jj);
#pragma unroll
                        for (int j = 1; j + 1 < QB; j += 2) m = kmax3(m, key_of(rb, j, jj), key_of(rb, j + 1, jj));
                        if (QB % 2 == 0) m = fmaxf(m, key_of(rb, QB - 1, jj));
                        hit |= MODE == 0 ? m > th[rb][jj] : m >= th[rb][jj];
                    }
                if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
                    // the start of every block and the diagonal come here; later only what tightens a list.  Only THIS wave pays
#pragma unroll
                    for (int j = 0; j < QB; ++j) {
                        const uint32_t col = c * (uint32_t)CH + (uint32_t)(16 * j + c16);
#pragma unroll
                        for (int rb = 0; rb < 2; ++rb) {
                            float key[4];
                            bool in[4];
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) {
                                key[jj] = key_of(rb, j, jj);
                                in[jj] = MODE == 0 ? key[jj] > th[rb][jj] : key[jj] >= th[rb][jj];
                            }
                            if (__builtin_amdgcn_ballot_w64(in[0] || in[1] || in[2] || in[3]) == 0ull) continue;  // wave-uniform
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) {
                                const uint32_t rl = (uint32_t)(16 * rb + 4 * kg + jj);
                                const uint32_t row = row0 + rl;
                                // (a fold inside an earlier append may have raised th: the list's own test decides again)
                                append(in[jj] && row < n_rows && col < n_rows && col != row, MODE == 0 ? rl : row, col, key[jj]);
                            }
                        }
                    }
                }
            }
            if (NBUF == 2) {
                __syncthreads();  // the other buffer is written, this one consumed
                buf ^= 1;
            }
        }

        if (MODE == 0 && active) {  // the block's lists -> the range's seeds
            fold();
            const uint32_t row = row0 + (uint32_t)lane;
            if (lane < 32 && row < n_rows) {
                for (uint32_t i = 0; i < k; ++i)
                    seeds[(size_t)(row - row_base) * k + i] = i < l_cnt ? my_lpos[i * 32 + lane] : 0xFFFFFFFFu;
            }
        }
    }
    if (MODE == 1 && my_cnt) flush_wave();
}

template <int METRIC>
__device__ __forceinline__ double exact_score(const double* __restrict__ x, const double* __restrict__ y, uint32_t dim)
{
    Acc64<METRIC> A;
    A.init();
    for (uint32_t c = 0; c < dim; ++c) A.step(x[c], y[c]);
    return A.score();
}

__device__ __forceinline__ KnnPay pay_of(double sc, uint32_t partner)
{
    return KnnPay{~assign_score_enc(sc), partner, (unsigned long long)__double_as_longlong(sc) == 0x8000000000000000ull ? 1u : 0u};
}

// 32 threads per row of the range, one per seed: the seed's reference score (row p the query) as a record; S = the k-th
// largest of them in the contract's order; thr = the join's threshold for min_score = S (-inf: no key is provably out).
template <int METRIC>
__global__ __launch_bounds__(256) void k_knn_seed(const double* __restrict__ master, uint32_t n_rows, uint32_t dim, uint32_t ldb,
                                                  uint32_t row_base, uint32_t range_rows, uint32_t k, double R, KnnRows rows,
                                                  uint32_t* __restrict__ ctr)
{
    const uint32_t i = blockIdx.x * 8 + (threadIdx.x >> 5);
    const uint32_t t = threadIdx.x & 31u;
    if (i >= range_rows) return;  // (whole groups of 32 lanes)
    const uint32_t row = row_base + i;
    const size_t rec = (size_t)i * k + t;
    if (row >= n_rows) {  // the padding of the last block: no key reaches +inf, the records sort last
        if (t == 0) rows.thr[i] = INFINITY;
        if (t < k) {
            rows.rec_keys[rec] = ~0ull;
            rows.rec_pay[rec] = KnnPay{~0ull, 0xFFFFFFFFu, 0u};
        }
        return;
    }
    unsigned long long enc = ~0ull;
    if (t < k) {
        const uint32_t col = rows.seeds[rec];
        if (col < n_rows && col != row) {
            const double sc = exact_score<METRIC>(master + (size_t)col * dim, master + (size_t)row * dim, dim);
            if (sc != sc) ctr[KNN_CTR_NAN] = 1u;
            enc = assign_score_enc(sc);
            rows.rec_keys[rec] = (unsigned long long)row;
            rows.rec_pay[rec] = pay_of(sc, col);
        } else {
            rows.rec_keys[rec] = ~0ull;
            rows.rec_pay[rec] = KnnPay{~0ull, 0xFFFFFFFFu, 0u};
        }
    }
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const unsigned long long o = __shfl_xor(enc, off);
        enc = o < enc ? o : enc;
    }
    if (t != 0) return;
    float th = -INFINITY;
    if (enc != ~0ull) {
        const double S = assign_score_dec(enc);
        const RangeKeys r = METRIC == COSINE ? join_key_threshold(ldb, S, &th) : join_pair_threshold(METRIC, ldb, R, S, &th);
        if (r == RANGE_KEYS_ALL) th = -INFINITY;
        if (S != S) th = -INFINITY;  // the call fails on the NaN flag
    }
    rows.thr[i] = th;
}

// the reference score of every kept pair, as the records behind the seeds'
template <int METRIC>
__global__ __launch_bounds__(256) void k_knn_pairs(const KnnCand* __restrict__ cand, uint32_t cap, const double* __restrict__ master,
                                                   uint32_t n_rows, uint32_t dim, uint32_t row_base, uint32_t range_rows, uint32_t k,
                                                   KnnRows rows, uint32_t* __restrict__ ctr)
{
    const uint32_t m = ctr[KNN_CTR_CAND];
    if (m > cap) return;  // the buffer is incomplete: the host splits the range
    const size_t rec0 = (size_t)range_rows * k;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < m; e += gridDim.x * 256) {
        const uint32_t row = cand[e].row, col = cand[e].col;
        if (row >= n_rows || row - row_base >= range_rows || col >= n_rows || col == row) {
            rows.rec_keys[rec0 + e] = ~0ull;
            rows.rec_pay[rec0 + e] = KnnPay{~0ull, 0xFFFFFFFFu, 0u};
            continue;
        }
        const double sc = exact_score<METRIC>(master + (size_t)col * dim, master + (size_t)row * dim, dim);
        if (sc != sc) ctr[KNN_CTR_NAN] = 1u;
        rows.rec_keys[rec0 + e] = (unsigned long long)row;
        rows.rec_pay[rec0 + e] = pay_of(sc, col);
    }
}

// One thread per row of the range: the start of its records by bisection, then the first kk distinct partners.  A seed that
// was also kept lies next to its copy (equal score bits, equal partner) and is emitted once.
__global__ __launch_bounds__(256) void k_knn_emit(uint32_t n_rows, uint32_t row_base, uint32_t range_rows, uint32_t kk,
                                                  unsigned long long total, KnnRows rows)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= range_rows || row_base + i >= n_rows) return;
    const unsigned long long row = row_base + i;
    unsigned long long lo = 0, hi = total;  // the first record whose key is >= row
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (rows.rec_keys[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    uint32_t n = 0;
    KnnPay prev{~0ull, 0xFFFFFFFFu, 0u};
    for (; lo < total && n < kk && rows.rec_keys[lo] == row; ++lo) {
        const KnnPay p = rows.rec_pay[lo];
        if (p == prev) continue;
        prev = p;
        rows.out_pos[(size_t)i * kk + n] = p.partner;
        rows.out_scores[(size_t)i * kk + n] = p.neg_zero ? -0.0 : assign_score_dec(~p.dkey);
        ++n;
    }
    for (; n < kk; ++n) {
        rows.out_pos[(size_t)i * kk + n] = 0xFFFFFFFFu;
        rows.out_scores[(size_t)i * kk + n] = 0.0;
    }
}

struct RowsArgs {
    const void* slab;
    const float* row_nrm;
    uint32_t n_rows, n_chunks;
    AssignRange r;
    uint32_t k;
    float e32;
    KnnRows rows;
    KnnCand* cand;
    uint32_t* cnt;
    uint32_t cap, grid;
};

template <int KSTEPS, int METRIC, int MODE>
hipError_t launch_rows(hipStream_t s, const RowsArgs& x)
{
    hipLaunchKernelGGL((k_knn_rows<KSTEPS, METRIC, MODE>), dim3(x.grid), dim3(KN_NW * 64), 0, s,
                       reinterpret_cast<const unsigned char*>(x.slab), x.row_nrm, x.n_rows, x.n_chunks, x.r.b0, x.r.b1, x.k, x.e32,
                       x.rows.seeds, x.rows.thr, x.cand, x.cnt, x.cap);
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
    return n_rows >= 2 && n_rows < 0xFFFFFFE0ull && r.b0 < r.b1 && (uint64_t)r.b1 <= (n_rows + KNN_BLOCK_ROWS - 1) / KNN_BLOCK_ROWS;
}

}  // namespace

bool knn_rows_supported(uint32_t dim, int metric)
{
    const uint32_t ldb = mfma_ldb(dim);
    if (metric != COSINE && metric != EUCLIDEAN && metric != DOT) return false;
    return dim >= 1 && (ldb == 128 || ldb == 256 || ldb == 384 || ldb == 512 || ldb == 768) && mfma_rows_kernel(dim);
}

hipError_t launch_knn_rows(hipStream_t s, int metric, int mode, const void* slab_frag, const float* row_norm, uint64_t n_rows,
                           uint32_t dim, AssignRange r, uint32_t k, const KnnRows& rows, KnnCand* cand, uint32_t cap, uint32_t* ctr)
{
    if (!knn_rows_supported(dim, metric) || !range_ok(r, n_rows) || !slab_frag || k < 1 || k > KNN_MAX_K || n_rows - 1 < k ||
        (mode != 0 && mode != 1))
        return hipErrorInvalidValue;
    if (metric != COSINE && !row_norm) return hipErrorInvalidValue;
    if (mode == 0 ? !rows.seeds : (!rows.thr || !cand || !ctr || cap == 0)) return hipErrorInvalidValue;
    const uint32_t ldb = mfma_ldb(dim);
    const uint32_t ch = knn_chunk(ldb);
    // one workgroup per CU (the buffers and lists fill its LDS); at least one 32-row block per wave
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus < 1) cus = 256;
    const uint32_t want = (r.b1 - r.b0 + KN_NW - 1) / KN_NW;
    const RowsArgs x{slab_frag, row_norm, (uint32_t)n_rows, (uint32_t)((n_rows + ch - 1) / ch), r, k, join_pair_e32(ldb), rows, cand,
                     ctr ? ctr + KNN_CTR_CAND : nullptr, cap, want < (uint32_t)cus ? want : (uint32_t)cus};
    switch (metric) {
    case COSINE: return launch_rows_mode<COSINE>(s, mode, ldb, x);
    case EUCLIDEAN: return launch_rows_mode<EUCLIDEAN>(s, mode, ldb, x);
    default: return launch_rows_mode<DOT>(s, mode, ldb, x);
    }
}

hipError_t launch_knn_seed(hipStream_t s, int metric, const double* master, uint64_t n_rows, uint32_t dim, AssignRange r, uint32_t k,
                           double R, const KnnRows& rows, uint32_t* ctr)
{
    if (!range_ok(r, n_rows) || k < 1 || k > KNN_MAX_K || !master || !ctr) return hipErrorInvalidValue;
    const uint32_t range_rows = (r.b1 - r.b0) * KNN_BLOCK_ROWS, row_base = r.b0 * KNN_BLOCK_ROWS, ldb = mfma_ldb(dim);
    const dim3 grid((range_rows + 7) / 8);
#define VL_KNN_SEED(M) \
    hipLaunchKernelGGL(k_knn_seed<M>, grid, dim3(256), 0, s, master, (uint32_t)n_rows, dim, ldb, row_base, range_rows, k, R, rows, ctr)
    switch (metric) {
    case COSINE: VL_KNN_SEED(COSINE); break;
    case EUCLIDEAN: VL_KNN_SEED(EUCLIDEAN); break;
    case DOT: VL_KNN_SEED(DOT); break;
    default: return hipErrorInvalidValue;
    }
#undef VL_KNN_SEED
    return hipGetLastError();
}

hipError_t launch_knn_pairs(hipStream_t s, int metric, const double* master, uint64_t n_rows, uint32_t dim, AssignRange r, uint32_t k,
                            const KnnRows& rows, const KnnCand* cand, uint32_t cap, uint32_t* ctr)
{
    if (!range_ok(r, n_rows) || k < 1 || k > KNN_MAX_K || !master || !cand || !ctr || cap == 0) return hipErrorInvalidValue;
    const uint32_t range_rows = (r.b1 - r.b0) * KNN_BLOCK_ROWS, row_base = r.b0 * KNN_BLOCK_ROWS;
    const dim3 grid(4096);  // grid-stride over the device's own pair count
#define VL_KNN_PAIRS(M) \
    hipLaunchKernelGGL(k_knn_pairs<M>, grid, dim3(256), 0, s, cand, cap, master, (uint32_t)n_rows, dim, row_base, range_rows, k, rows, ctr)
    switch (metric) {
    case COSINE: VL_KNN_PAIRS(COSINE); break;
    case EUCLIDEAN: VL_KNN_PAIRS(EUCLIDEAN); break;
    case DOT: VL_KNN_PAIRS(DOT); break;
    default: return hipErrorInvalidValue;
    }
#undef VL_KNN_PAIRS
    return hipGetLastError();
}

hipError_t launch_knn_emit(hipStream_t s, uint64_t n_rows, AssignRange r, uint32_t kk, uint64_t total, const KnnRows& rows)
{
    if (!range_ok(r, n_rows) || kk < 1 || kk > KNN_MAX_K || total == 0) return hipErrorInvalidValue;
    const uint32_t range_rows = (r.b1 - r.b0) * KNN_BLOCK_ROWS, row_base = r.b0 * KNN_BLOCK_ROWS;
    hipLaunchKernelGGL(k_knn_emit, dim3((range_rows + 255) / 256), dim3(256), 0, s, (uint32_t)n_rows, row_base, range_rows, kk,
                       (unsigned long long)total, rows);
    return hipGetLastError();
}

}  // namespace vl
