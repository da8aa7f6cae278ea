// deep_batch.hip -- the deep-k batch: query batches with KFAST_MAX < k <= VL_DEEP_MAX_K.
//
// k_deep_sample<KSTEPS, METRIC> makes the bootstrap threshold's input on the matrix cores (v_mfma_f32_16x16x32_bf16):
//   A = 32-row blocks of the fragment-major slab, one block per wave at a time, its fragments in registers -- the whole K
//       of stride 128, above it in phases of 4 K-steps that refill the same registers (no shape uses scratch);
//   B = the workgroup's query chunk (the chunk of k_mfma_rows: 128 queries, 96 at stride 768), copied once into the padded
//       LDS image k_mfma_rows keeps its queries in (row stride + 32 bytes: conflict-free ds_read_b128);
//   C = one 16 x 16 tile per (row half, query block): a lane holds four consecutive rows of one query, so the maximum of
//       its four registers and the matching four of the block's other half is the maximum over 8 rows of the block with no
//       cross-lane traffic.  A block leaves the kernel as 4 group maxima per query, stored group-major (16 neighbouring
//       lanes write 16 neighbouring queries).
// The K-th largest of G maxima of DISJOINT groups is reached by K distinct rows: a lower bound of the K-th best key.
//
// k_deep_select (one workgroup per query) returns the K-th largest of up to 16 384 f32 keys by radix selection on the
// order-preserving u32 image -- the keys go to LDS once, four 8-bit digit passes fill a 256-bin LDS histogram in which a
// wave adds each digit it holds ONCE (ballots find the lanes that share a digit, the lowest of them adds their number) --
// and moves every entry that reaches the result to the front of the buffer, ties included.
#include "deep_batch.hpp"

#include <cmath>

#include "device_common.hpp"
#include "mfma_scan.hpp"

namespace vl {

using namespace dev;
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int DS_NW = 8;  // waves per workgroup of the sampling pass
constexpr int deep_qpb(int ldb) { return ldb <= 512 ? 128 : 96; }

// max of three floats that are MFMA sums of finite bf16 products, finite per-row scalars applied, or -inf: one
// instruction (fmaxf() canonicalises each operand first in IEEE mode)
__device__ __forceinline__ float max3f(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

template <int KSTEPS, int METRIC>
__global__ __launch_bounds__(DS_NW * 64) void k_deep_sample(const __bf16* __restrict__ slab16, const float* __restrict__ row_nrm,
                                                           const float* __restrict__ row_sqn, const __bf16* __restrict__ q16,
                                                           uint32_t nq_pad, uint32_t sample_blocks, uint32_t n_blk, uint32_t n_rows,
                                                           float* __restrict__ gm)
{
    constexpr int LDB = KSTEPS * 16;
    constexpr int ROW_BYTES = LDB * 2;
    constexpr int LDS_ROW = ROW_BYTES + 32;
    constexpr int KS32 = KSTEPS / 2;  // K = 32 per MFMA
    constexpr int KSP = 4;            // K-steps per phase = row fragments held per 16-row half (a row of stride 128 is one phase)
    constexpr int PH = KS32 / KSP;
    constexpr int QPB = deep_qpb(LDB);
    constexpr int QB = QPB / 16;
    constexpr int NT = DS_NW * 64;
    static_assert(KSTEPS % 2 == 0 && KS32 % KSP == 0, "whole 32-deep K steps in whole phases");

    __shared__ __attribute__((aligned(16))) unsigned char q_lds[QPB * LDS_ROW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, kg = lane >> 4;
    const uint32_t chunk_base = blockIdx.y * QPB;  // the launcher pads nq_pad to whole chunks
    {
        constexpr int CPR = ROW_BYTES / 16;
        constexpr int PIECES = QPB * CPR;
        const unsigned char* src = reinterpret_cast<const unsigned char*>(q16) + (size_t)chunk_base * ROW_BYTES;
        for (int c = tid; c < PIECES; c += NT) {
            const int r = c / CPR, cc = c % CPR;
            *reinterpret_cast<u32x4*>(&q_lds[r * LDS_ROW + cc * 16]) = *reinterpret_cast<const u32x4*>(src + (size_t)c * 16);
        }
    }
    __syncthreads();

    const unsigned char* qrow = &q_lds[c16 * LDS_ROW + kg * 16];
    for (uint32_t i = blockIdx.x + gridDim.x * (uint32_t)wave; i < sample_blocks; i += gridDim.x * DS_NW) {  // wave-uniform
        const uint32_t blk = deep_sample_block(i, sample_blocks, n_blk);
        const uint32_t row0 = blk * 32u;
        // fragment (rb, s) of a block is one contiguous 1 KB wave load (k_rows_bf16_frag's layout)
        const unsigned char* pa = reinterpret_cast<const unsigned char*>(slab16) + (size_t)blk * (32 * ROW_BYTES) + (uint32_t)lane * 16u;
        f32x4 acc[2][QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) acc[0][j] = acc[1][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ph = 0; ph < PH; ++ph) {
            bf16x8 a[2][KSP];
#pragma unroll
            for (int s = 0; s < KSP; ++s)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
                    a[rb][s] = *reinterpret_cast<const bf16x8*>(pa + rb * (16 * ROW_BYTES) + (ph * KSP + s) * 1024);
#pragma unroll
            for (int s = 0; s < KSP; ++s)
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const bf16x8 b = *reinterpret_cast<const bf16x8*>(qrow + j * 16 * LDS_ROW + (ph * KSP + s) * 64);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][s], b, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][s], b, acc[1][j], 0, 0, 0);
                    // (left alone the compiler reads every step's query fragments in front of the first MFMA and spills)
                    if (j % 4 == 3) __builtin_amdgcn_sched_barrier(0);
                }
        }
        // ---- epilogue: C layout of a 16 x 16 tile: column = lane & 15 (query), row = 4 (lane >> 4) + register ----
        f32x4 nrm[2] = {f32x4{1.f, 1.f, 1.f, 1.f}, f32x4{1.f, 1.f, 1.f, 1.f}};
        f32x4 sqn[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {  // (the per-row arrays are allocated in whole tiles of 64 rows, like the slab)
            const uint32_t r0 = row0 + 16 * rb + 4 * kg;
            if (METRIC != COSINE) nrm[rb] = *reinterpret_cast<const f32x4*>(row_nrm + r0);
            if (METRIC == EUCLIDEAN) sqn[rb] = *reinterpret_cast<const f32x4*>(row_sqn + r0);
        }
        const bool partial = row0 + 32u > n_rows;  // wave-uniform: only the index's last block
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            float key[2][4];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float v = acc[rb][j][jj];                                         // cosine: x^.q
                    if (METRIC == DOT) v *= nrm[rb][jj];                              // x.q
                    if (METRIC == EUCLIDEAN) v = 2.0f * v * nrm[rb][jj] - sqn[rb][jj];  // |q|^2 - |x - q|^2
                    if (partial && row0 + (uint32_t)(16 * rb + 4 * kg + jj) >= n_rows) v = -INFINITY;
                    key[rb][jj] = v;
                }
            // the 8 rows {4 kg .. 4 kg + 3} of both halves: a group no other lane, block or launch shares
            float m = max3f(key[0][0], key[0][1], key[0][2]);
            m = max3f(m, key[0][3], key[1][0]);
            m = max3f(m, key[1][1], key[1][2]);
            m = max3f(m, key[1][3], key[1][3]);
            gm[(size_t)(4u * i + (uint32_t)kg) * nq_pad + chunk_base + (uint32_t)(j * 16 + c16)] = m;
        }
    }
}

// ---- selection ---------------------------------------------------------------------------------------------------------
constexpr int SEL_NT = 1024;

__device__ __forceinline__ uint32_t key_image(float f)  // unsigned order = float order
{
    const uint32_t b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float image_key(uint32_t u) { return __uint_as_float((u >> 31) ? (u & 0x7FFFFFFFu) : ~u); }

// The K-th largest of keys[0 .. n) (LDS, images), 1 <= K <= n.  hist: 256 words, sh: 2 words.  Every thread of the
// workgroup calls it; it begins and ends with the keys readable by all.
__device__ uint32_t radix_kth(const uint32_t* keys, uint32_t n, uint32_t K, uint32_t* hist, uint32_t* sh)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t prefix = 0, pmask = 0, need = K;
    const uint32_t n_round = (n + SEL_NT - 1) / SEL_NT * SEL_NT;  // whole waves take every trip: the ballots see 64 lanes
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (uint32_t i = tid; i < 256u; i += SEL_NT) hist[i] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n_round; i += SEL_NT) {
            const uint32_t u = i < n ? keys[i] : 0u;
            const bool live = i < n && (u & pmask) == prefix;
            const uint32_t d = (u >> shift) & 255u;
            unsigned long long peers = __ballot(live);  // ... the live lanes that hold this lane's digit
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const unsigned long long bal = __ballot(bit);
                peers &= bit ? bal : ~bal;
            }
            if (live && (peers & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&hist[d], (uint32_t)__popcll(peers));
        }
        __syncthreads();
        if (tid < 64u) {  // the bin that holds the need-th largest: a suffix sum over the lanes' four bins each
            const uint32_t h[4] = {hist[4 * lane], hist[4 * lane + 1], hist[4 * lane + 2], hist[4 * lane + 3]};
            const uint32_t sum = h[0] + h[1] + h[2] + h[3];
            uint32_t incl = sum;
            for (uint32_t o = 1; o < 64u; o <<= 1) {
                const uint32_t v = __shfl_down(incl, o);
                if (lane + o < 64u) incl += v;
            }
            const uint32_t excl = incl - sum;  // keys in the bins above this lane's
            if (excl < need && need <= incl) {  // exactly one lane
                uint32_t above = excl;
                int b = 3;
                for (; b > 0; --b) {
                    if (above + h[b] >= need) break;
                    above += h[b];
                }
                sh[0] = 4u * lane + (uint32_t)b;
                sh[1] = need - above;
            }
        }
        __syncthreads();
        prefix |= sh[0] << shift;
        pmask |= 255u << shift;
        need = sh[1];
        __syncthreads();
    }
    return prefix;
}

__global__ __launch_bounds__(SEL_NT) void k_deep_select_sample(const float* __restrict__ gm, uint32_t nq_pad, uint32_t n_groups,
                                                              uint32_t K, const float* __restrict__ mask, float* __restrict__ thr)
{
    __shared__ uint32_t keys[DEEP_SELECT_MAX];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[2];
    const uint32_t q = blockIdx.x;
    if (n_groups == 0 || K == 0 || K > n_groups) {  // no sample: the first stage keeps every row
        if (threadIdx.x == 0) thr[q] = mask[q];
        return;
    }
    for (uint32_t g = threadIdx.x; g < n_groups; g += SEL_NT) keys[g] = key_image(gm[(size_t)g * nq_pad + q]);
    __syncthreads();
    const float t = image_key(radix_kth(keys, n_groups, K, hist, sh));
    if (threadIdx.x == 0) thr[q] = t > mask[q] ? t : mask[q];
}

__global__ __launch_bounds__(SEL_NT) void k_deep_select(const Cand32* cand, uint32_t* cnt, uint32_t cap, uint32_t K,
                                                       float* __restrict__ thr, int write_thr, Cand32* dst, uint32_t* dst_cnt,
                                                       uint32_t dst_cap)
{
    __shared__ uint32_t keys[DEEP_SELECT_MAX];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[2];
    __shared__ uint32_t wsum[SEL_NT / 64];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = cnt[q];  // workgroup-uniform
    const bool in_place = dst == cand;
    if (n > cap) {  // the buffer or a ring segment overflowed: the host redoes the query
        if (tid == 0) {
            if (write_thr) thr[q] = INFINITY;
            if (!in_place) dst_cnt[q] = dst_cap + 1u;
        }
        return;
    }
    const Cand32* mine = cand + (size_t)q * cap;
    Cand32* out = dst + (size_t)q * dst_cap;
    float T = thr[q];
    if (K > 0) {
        if (n < K) {  // not K entries yet: the threshold and the buffer stand
            if (!in_place && tid == 0) dst_cnt[q] = 0u;
            return;
        }
        for (uint32_t i = tid; i < n; i += SEL_NT) keys[i] = key_image(mine[i].key);
        __syncthreads();
        T = image_key(radix_kth(keys, n, K, hist, sh));
        if (write_thr && tid == 0) thr[q] = T;
    }
    // entries with key >= T to the front, in their order.  In place: an entry moves to an index at or below its own, and a
    // trip's entries are all read before the first of them is written.
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += SEL_NT) {  // workgroup-uniform
        const uint32_t i = i0 + tid;
        Cand32 e;
        e.key = 0.0f;
        e.pos = 0u;
        bool keep = false;
        if (i < n) {
            e = mine[i];
            keep = e.key >= T;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base, total = 0;
        for (uint32_t w = 0; w < SEL_NT / 64; ++w) {
            const uint32_t c = wsum[w];
            if (w < wave) off += c;
            total += c;
        }
        const uint32_t slot = off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (keep && slot < dst_cap) out[slot] = e;
        base += total;
        __syncthreads();
    }
    if (tid == 0) dst_cnt[q] = base <= dst_cap ? base : dst_cap + 1u;
}

__global__ __launch_bounds__(256) void k_deep_stripe(const float* __restrict__ thr, uint32_t nq, uint32_t qpb, uint32_t A, uint32_t a,
                                                    float* __restrict__ out)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q < nq) out[q] = ((q % qpb) % A == a) ? thr[q] : INFINITY;
}

// one wave per query
__global__ __launch_bounds__(256) void k_deep_seed_min(const double* __restrict__ scores, uint32_t seg, const uint32_t* __restrict__ ctr,
                                                      uint32_t ctr_words, uint32_t nq, double* __restrict__ L)
{
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (q >= nq) return;
    const uint32_t total = ctr[(size_t)q * ctr_words + RBATCH_CTR_TOTAL];
    const bool bad = total == 0u || total > seg || ctr[(size_t)q * ctr_words + RBATCH_CTR_NAN] != 0u;
    double m = INFINITY;
    if (!bad)
        for (uint32_t i = lane; i < total; i += 64u) {
            const double s = scores[(size_t)q * seg + i];
            m = s < m ? s : m;
        }
    for (int o = 32; o >= 1; o >>= 1) {
        const double v = __shfl_xor(m, o);
        m = v < m ? v : m;
    }
    if (lane == 0) L[q] = bad ? NAN : m;
}

__global__ __launch_bounds__(256) void k_deep_clear(uint32_t* __restrict__ words, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) words[i] = 0u;
}

}  // namespace

bool deep_sample_supported(uint32_t dim, int metric)
{
    if (metric != COSINE && metric != DOT && metric != EUCLIDEAN) return false;
    const uint32_t ldb = mfma_ldb(dim);
    return ldb == 128 || ldb == 256 || ldb == 384 || ldb == 512 || ldb == 768;
}

hipError_t launch_deep_sample(hipStream_t s, int metric, const void* slab_frag, const float* row_norm, const float* row_sqnorm,
                              const void* q_bf16, uint32_t nq_pad, uint32_t sample_blocks, uint64_t n_rows, uint32_t dim, float* gm)
{
    if (!deep_sample_supported(dim, metric) || n_rows == 0 || n_rows >= 0xFFFFFFE0ull || sample_blocks == 0) return hipErrorInvalidValue;
    const uint32_t ldb = mfma_ldb(dim);
    const uint32_t qpb = (uint32_t)deep_qpb((int)ldb);
    const uint32_t n_blk = (uint32_t)((n_rows + 31) / 32);
    if (nq_pad == 0 || nq_pad % qpb != 0 || sample_blocks > n_blk || 4ull * sample_blocks > DEEP_SELECT_MAX) return hipErrorInvalidValue;
    const uint32_t chunks = nq_pad / qpb;
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const uint32_t gx = std::max<uint32_t>(1u, std::min<uint32_t>((sample_blocks + DS_NW - 1) / DS_NW, (uint32_t)cus / chunks + 1u));
    const __bf16* slab = reinterpret_cast<const __bf16*>(slab_frag);
    const __bf16* q16 = reinterpret_cast<const __bf16*>(q_bf16);
#define VL_DEEP_GO(K, MET)                                                                                                       \
    hipLaunchKernelGGL((k_deep_sample<K, MET>), dim3(gx, chunks), dim3(DS_NW * 64), 0, s, slab, row_norm, row_sqnorm, q16, nq_pad, \
                       sample_blocks, n_blk, (uint32_t)n_rows, gm);
#define VL_DEEP_K(K)                                      \
    if (ldb == (uint32_t)(K * 16)) {                      \
        if (metric == COSINE) VL_DEEP_GO(K, COSINE)       \
        else if (metric == EUCLIDEAN) VL_DEEP_GO(K, EUCLIDEAN) \
        else VL_DEEP_GO(K, DOT)                           \
    }
    VL_DEEP_K(8) VL_DEEP_K(16) VL_DEEP_K(24) VL_DEEP_K(32) VL_DEEP_K(48)
#undef VL_DEEP_K
#undef VL_DEEP_GO
    return hipGetLastError();
}

hipError_t launch_deep_select_sample(hipStream_t s, const float* gm, uint32_t nq_pad, uint32_t n_groups, uint32_t K, uint32_t nq,
                                     const float* mask, float* thr)
{
    if (nq == 0 || n_groups > DEEP_SELECT_MAX || !mask || !thr || (n_groups && !gm)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deep_select_sample, dim3(nq), dim3(SEL_NT), 0, s, gm, nq_pad, n_groups, K, mask, thr);
    return hipGetLastError();
}

hipError_t launch_deep_select(hipStream_t s, const Cand32* cand, uint32_t* cnt, uint32_t cap, uint32_t nq, uint32_t K, float* thr,
                              bool write_thr, Cand32* dst, uint32_t* dst_cnt, uint32_t dst_cap)
{
    if (nq == 0 || cap == 0 || cap > DEEP_SELECT_MAX || dst_cap == 0 || !cand || !cnt || !thr || !dst || !dst_cnt) return hipErrorInvalidValue;
    if ((dst == cand) != (dst_cnt == cnt) || (dst == cand && dst_cap != cap)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deep_select, dim3(nq), dim3(SEL_NT), 0, s, cand, cnt, cap, K, thr, write_thr ? 1 : 0, dst, dst_cnt, dst_cap);
    return hipGetLastError();
}

hipError_t launch_deep_stripe(hipStream_t s, const float* thr, uint32_t nq, uint32_t qpb, uint32_t A, uint32_t a, float* out)
{
    if (nq == 0 || qpb == 0 || A == 0 || a >= A) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deep_stripe, dim3((nq + 255) / 256), dim3(256), 0, s, thr, nq, qpb, A, a, out);
    return hipGetLastError();
}

hipError_t launch_deep_seed_min(hipStream_t s, const double* scores, uint32_t seg, const uint32_t* ctr, uint32_t ctr_words,
                                uint32_t nq, double* L)
{
    if (nq == 0 || seg == 0 || ctr_words <= (uint32_t)RBATCH_CTR_NAN) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deep_seed_min, dim3((nq + 3) / 4), dim3(256), 0, s, scores, seg, ctr, ctr_words, nq, L);
    return hipGetLastError();
}

hipError_t launch_deep_clear(hipStream_t s, uint32_t* words, uint32_t n)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_deep_clear, dim3((n + 255) / 256), dim3(256), 0, s, words, n);
    return hipGetLastError();
}

}  // namespace vl
