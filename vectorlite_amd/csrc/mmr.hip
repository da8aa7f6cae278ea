// mmr.hip -- the tail of a diversified (maximal marginal relevance) search, DESIGN.md section 16: the pairwise reference
// similarities of a search's finalised candidates and the greedy selection over them.  Both kernels read the candidates
// where the search's last kernel left them in device memory and decide on the device whether there is anything to do,
// so nothing stands between the search's finalize and the answer but two launches.
#include "device_common.hpp"
#include "score_bound.hpp"

#include <type_traits>

namespace vl {

using namespace dev;

namespace {

// Candidates the search certified (or computed exactly), 0 when it did not: the host then reads NEEDS_EXACT (fast
// routes: down the ladder) or the exact scan's NaN flag and never looks at the selection.
__device__ __forceinline__ uint32_t mmr_count(const MmrSource& s)
{
    if (s.nan_flag && *s.nan_flag) return 0u;
    if (s.blocks) {
        const uint32_t flags = s.blocks[0].flags;
        if (s.blocks[0].n_out != s.n_block0 || (flags & (RESULT_NEEDS_EXACT | RESULT_HAS_NAN))) return 0u;
    }
    return s.n <= MMR_MAX_FETCH ? s.n : 0u;
}

// candidate i's storage position (clamped into the index: a row is read from it) and reference score
__device__ __forceinline__ uint32_t mmr_pos(const MmrSource& s, uint32_t i)
{
    uint32_t p = s.blocks ? s.blocks[i / KP].pos[i % KP] : s.pos[i];
    if (s.plist) p = p < s.plist_len ? s.plist[p] : 0u;
    return p < s.n_rows ? p : 0u;
}
__device__ __forceinline__ double mmr_rel(const MmrSource& s, uint32_t i)
{
    return s.blocks ? s.blocks[i / KP].score[i % KP] : s.scores[i];
}

constexpr int PW_T = 16;   // a workgroup owns a PW_T x PW_T tile of pairs, one pair per thread
constexpr int PW_CH = 32;  // columns of the 2 x PW_T rows staged per step

// sim[i][j] = sim[j][i] = calculate(metric, row[i], row[j]) for i < j < n: one serial f64 chain per pair in index order
// (Acc64: separate multiply and add, k_exact_scan's tail).  The grid runs over the upper triangle's tiles, (bi <= bj);
// the rows of a tile are staged chunk by chunk through LDS, the next chunk's loads in flight during the arithmetic.
template <int METRIC>
__global__ __launch_bounds__(256) void k_mmr_pairwise(const double* __restrict__ master, uint32_t dim, MmrSource src,
                                                      double* __restrict__ sim)
{
    __shared__ double ta[PW_T][PW_CH + 1];
    __shared__ double tb[PW_T][PW_CH + 1];
    const uint32_t n = mmr_count(src);
    if (n < 2u) return;
    // blockIdx.x -> (bi, bj), bi <= bj < tiles_max (the host sized the grid for src.n)
    const uint32_t tiles = (n + PW_T - 1) / PW_T;
    uint32_t bi = 0, rest = blockIdx.x;
    while (bi < tiles && rest >= tiles - bi) {
        rest -= tiles - bi;
        ++bi;
    }
    if (bi >= tiles) return;
    const uint32_t bj = bi + rest;
    const int tid = threadIdx.x;
    const uint32_t ti = (uint32_t)tid / PW_T, tj = (uint32_t)tid % PW_T;
    const uint32_t gi = bi * PW_T + ti, gj = bj * PW_T + tj;

    // what this thread stages: 2 x PW_T rows x PW_CH columns = 1024 values, 4 per thread; slot -> (row of a | b, column)
    constexpr int PER = 2 * PW_T * PW_CH / 256;
    uint64_t base[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const uint32_t r = (uint32_t)(tid + e * 256) / PW_CH;  // 0 .. 2 PW_T - 1
        uint32_t g = r < (uint32_t)PW_T ? bi * PW_T + r : bj * PW_T + (r - PW_T);
        g = g < n ? g : n - 1u;  // clamped, never predicated: the pairs of such rows are not stored
        base[e] = (uint64_t)mmr_pos(src, g) * dim;
    }
    double pre[PER];
    auto fetch = [&](uint32_t c0) {
        const uint32_t cw = (dim - c0) < (uint32_t)PW_CH ? (dim - c0) : (uint32_t)PW_CH;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            uint32_t cc = (uint32_t)(tid + e * 256) % PW_CH;
            cc = cc < cw ? cc : cw - 1u;  // columns >= cw are never stepped
            pre[e] = master[base[e] + c0 + cc];
        }
    };
    Acc64<METRIC> A;
    A.init();
    const uint32_t n_chunks = (dim + PW_CH - 1) / PW_CH;
    if (n_chunks) fetch(0);
    for (uint32_t ch = 0; ch < n_chunks; ++ch) {
        const uint32_t c0 = ch * PW_CH;
        const uint32_t cw = (dim - c0) < (uint32_t)PW_CH ? (dim - c0) : (uint32_t)PW_CH;
        __syncthreads();  // the previous chunk's readers are done with the tiles
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const uint32_t r = (uint32_t)(tid + e * 256) / PW_CH, cc = (uint32_t)(tid + e * 256) % PW_CH;
            if (r < (uint32_t)PW_T)
                ta[r][cc] = pre[e];
            else
                tb[r - PW_T][cc] = pre[e];
        }
        __syncthreads();
        if (ch + 1 < n_chunks) fetch(c0 + PW_CH);
        if (cw == (uint32_t)PW_CH) {
#pragma unroll
            for (uint32_t cc = 0; cc < (uint32_t)PW_CH; ++cc) A.step(ta[ti][cc], tb[tj][cc]);
        } else {
            for (uint32_t cc = 0; cc < cw; ++cc) A.step(ta[ti][cc], tb[tj][cc]);
        }
    }
    if (gi < gj && gj < n) {
        const double s = A.score();
        sim[(size_t)gi * MMR_MAX_FETCH + gj] = s;
        sim[(size_t)gj * MMR_MAX_FETCH + gi] = s;  // the four metrics are symmetric bit for bit
    }
}

// argmax candidate of the selection's round: valid entries order by (value desc, rank asc)
__device__ __forceinline__ void mmr_take_better(double& v, uint32_t& idx, double ov, uint32_t oidx)
{
    const bool other = oidx != POS_SENTINEL && (idx == POS_SENTINEL || ov > v || (ov == v && oidx < idx));
    if (other) {
        v = ov;
        idx = oidx;
    }
}

// The greedy selection, one workgroup, thread i = candidate i.  Each of the min(k, n) - 1 rounds folds the column of the
// candidate chosen last into red[], computes v = (lambda * rel) - ((1 - lambda) * red) with individually rounded
// operations and takes the block argmax under the contract's scan: the first unselected candidate wins unless a later
// one has a strictly larger v; a NaN v never beats anything (so it wins only as that first candidate).  The chosen
// candidates' (storage position, score bits) go to the result blocks in selection order, 64 per block, the count and
// the flags to block 0, the stamp last.
__global__ __launch_bounds__(MMR_MAX_FETCH) void k_mmr_select(MmrSource src, const double* __restrict__ sim, uint32_t k,
                                                              double lambda, SearchResultBlock* __restrict__ out, uint32_t seq)
{
    constexpr int NW = MMR_MAX_FETCH / WAVE;
    __shared__ double rel[MMR_MAX_FETCH];
    __shared__ double red[MMR_MAX_FETCH];
    __shared__ uint32_t chosen[MMR_MAX_FETCH];
    __shared__ double w_v[2][NW];
    __shared__ uint32_t w_idx[2][NW];
    __shared__ uint32_t w_first[2][NW];
    const uint32_t i = threadIdx.x;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const uint32_t n = mmr_count(src);
    const uint32_t n_sel = k < n ? k : n;
    const bool mine = i < n;
    uint32_t my_pos = 0u;
    rel[i] = 0.0;
    red[i] = neg_inf<double>();
    chosen[i] = 0u;
    if (mine) {
        my_pos = mmr_pos(src, i);
        rel[i] = mmr_rel(src, i);
    }
    const double one_minus = __dsub_rn(1.0, lambda);
    if (n_sel > 0u && i == 0u) {  // sel = [0]
        chosen[0] = 1u;
        out[0].pos[0] = my_pos;
        out[0].score[0] = rel[0];
    }
    uint32_t last = 0u;
    for (uint32_t t = 1; t < n_sel; ++t) {
        const int pp = (int)(t & 1u);
        double v = 0.0;
        uint32_t idx = POS_SENTINEL, first = POS_SENTINEL;
        if (mine && !chosen[i]) {
            const double s = sim[(size_t)last * MMR_MAX_FETCH + i];  // = sim[i][last], read along the row
            if (s > red[i]) red[i] = s;
            v = __dsub_rn(__dmul_rn(lambda, rel[i]), __dmul_rn(one_minus, red[i]));
            first = (i << 1) | (v != v ? 1u : 0u);  // the smallest code = the first unselected candidate, bit 0: its v is NaN
            if (v == v) idx = i;                    // a NaN takes no part in the comparison
        }
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const double ov = __shfl_xor(v, o);
            const uint32_t oidx = __shfl_xor(idx, o), ofirst = __shfl_xor(first, o);
            mmr_take_better(v, idx, ov, oidx);
            first = ofirst < first ? ofirst : first;
        }
        if (lane == 0) {
            w_v[pp][wave] = v;
            w_idx[pp][wave] = idx;
            w_first[pp][wave] = first;
        }
        __syncthreads();  // one barrier per round: the slots alternate, every thread folds the NW entries itself
        v = w_v[pp][0];
        idx = w_idx[pp][0];
        first = w_first[pp][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            mmr_take_better(v, idx, w_v[pp][w], w_idx[pp][w]);
            const uint32_t of = w_first[pp][w];
            first = of < first ? of : first;
        }
        // the first unselected candidate stands unless a later comparison `v > v_best` succeeds: with a NaN there none does
        uint32_t best = idx;
        if (first != POS_SENTINEL && (first & 1u)) best = first >> 1;
        if (best == POS_SENTINEL) break;  // (uniform; cannot happen while t < n)
        if (i == best) {
            chosen[i] = 1u;
            out[t / KP].pos[t % KP] = my_pos;
            out[t / KP].score[t % KP] = rel[i];
        }
        last = best;
    }
    __threadfence_system();  // every writer's entries are out before the count and the stamp
    __syncthreads();
    if (i == 0u) {
        out[0].n_out = n_sel;
        out[0].flags = n ? 0u : RESULT_NEEDS_EXACT;
        if (seq) {
            __threadfence_system();
            __hip_atomic_store(&out[0].seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The batched form: the stage behind k_batch_rescore in a launch sequence of the MFMA batch filter.
//   k_mmr_batch_rank    one wave per query: rank the 64 rescored candidates, certify the prefix scoring strictly above the
//                       bound of the list's 64th key, leave the first n ranked candidates in a device block
//   k_mmr_batch_select  one workgroup per query: the pairwise similarities of those n <= 60 candidates into LDS (eager:
//                       every pair), then the greedy selection in wave 0, lane i = candidate i
// ---------------------------------------------------------------------------------------------
constexpr int MB_N = KFAST_MAX;  // candidates of a settled query: n <= 60 of the 64-entry list
constexpr int MB_CH = 32;        // columns of the n rows staged per step
constexpr int MB_THREADS = 256;
constexpr int MB_PAIRS = (MB_N * (MB_N - 1) / 2 + MB_THREADS - 1) / MB_THREADS;  // chains a thread carries: 7
constexpr int MB_PER = KP * MB_CH / MB_THREADS;                                  // values a thread stages per step: 8
static_assert(MB_N <= KP && KP == WAVE, "lane i is candidate i");

// k_batch_rank_collapse's ranking and certificate.  The lists hold rows of S only and n_rows = |S|.  A candidate is
// CERTIFIED iff its score is > B = bound_for_key(the list's 64th key), strictly: no row outside the list scores above B,
// so the certified candidates are a prefix of S's ranking, exact and in order.  (A list that holds all n_rows <= 64 rows has
// no row outside it: every candidate is certified.)  Settled iff no score is NaN and the prefix holds n_need candidates;
// then ranked[q] = {n_out = n_need, flags = 0, (pos, score) by rank}.  Otherwise flags carries RESULT_NEEDS_EXACT.
template <int METRIC>
__global__ __launch_bounds__(256) void k_mmr_batch_rank(const Cand32* __restrict__ lists, const double* __restrict__ scores,
                                                        const double* __restrict__ q_norms, uint32_t nq, uint32_t ld,
                                                        uint64_t n_rows, uint32_t n_need, double R, double in_extra,
                                                        SearchResultBlock* __restrict__ ranked)
{
    const int lane = lane_id();
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const Cand32 e = lists[(size_t)q * KP + lane];
    const int n_cand = __popcll(__ballot(e.pos != POS_SENTINEL));
    const bool valid = lane < n_cand;
    const double sc = valid ? scores[(size_t)q * KP + lane] : 0.0;
    const uint32_t my_pos = e.pos;
    const bool any_nan = __ballot(valid && sc != sc) != 0ull;
    int rank = 0;  // (score desc, position asc), as rank_check_emit ranks
    for (int j = 0; j < n_cand; ++j) {
        const double sj = read_lane(sc, j);
        const uint32_t pj = read_lane(my_pos, j);
        rank += (sj > sc || (sj == sc && pj < my_pos)) ? 1 : 0;
    }
    uint32_t flags = 0;
    if (any_nan) flags |= RESULT_HAS_NAN | RESULT_NEEDS_EXACT;
    bool certified = false;
    if (n_rows <= (uint64_t)KP) {
        const bool complete = (uint64_t)n_cand >= n_rows;  // the list is the whole of S
        if (!complete) flags |= RESULT_NEEDS_EXACT;
        certified = valid && complete && !any_nan;
    } else if (n_cand < KP) {
        flags |= RESULT_NEEDS_EXACT;  // keys were not finite, or the candidate stage dropped rows
    } else {
        const double B = bound_for_key<METRIC>(read_lane(e.key, KP - 1), ld, R, q_norms[q], in_extra);
        certified = !any_nan && sc > B;
    }
    const uint32_t n_cert = (uint32_t)__popcll(__ballot(certified));
    if (n_cert < n_need) flags |= RESULT_NEEDS_EXACT;
    SearchResultBlock* o = ranked + q;
    if (flags == 0u && valid && (uint32_t)rank < n_need) {
        o->pos[rank] = my_pos;
        o->score[rank] = sc;
    }
    if (lane == 0) {
        o->n_out = flags == 0u ? n_need : 0u;
        o->flags = flags;
    }
}

// One workgroup per query.  ranked[q] unsettled: the flags go to out[q] and nothing else happens.  Otherwise n = n_out
// candidates in rank order, n_sel = min(k, n) of them are chosen:
//   sim[i][j] = sim[j][i] = calculate(metric, row[i], row[j]), i < j < n, as k_mmr_pairwise computes it: one serial Acc64
//   chain per pair in index order, x = the row of smaller rank; the n master rows are staged through LDS MB_CH columns at a
//   time, the next chunk's loads in flight during the arithmetic; a thread carries up to MB_PAIRS chains (pair p of the
//   upper triangle in row-major order belongs to thread p % MB_THREADS).  Skipped when n_sel < 2.
//   Then wave 0 runs k_mmr_select's rounds with lane i = candidate i: no barrier per round.  The chosen candidates'
//   (storage position, score bits) go to out[q] in selection order, the count and the flags last.
template <int METRIC>
__global__ __launch_bounds__(MB_THREADS) void k_mmr_batch_select(const double* __restrict__ master, uint32_t dim,
                                                                 uint32_t index_rows,
                                                                 const SearchResultBlock* __restrict__ ranked, uint32_t k,
                                                                 double lambda, SearchResultBlock* __restrict__ out)
{
    __shared__ double sim[MB_N][MB_N];
    __shared__ double tile[KP][MB_CH + 1];
    const uint32_t q = blockIdx.x;
    const SearchResultBlock* in = ranked + q;
    SearchResultBlock* o = out + q;
    const int tid = threadIdx.x;
    const uint32_t in_flags = in->flags;
    const uint32_t n = in->n_out;
    if (in_flags != 0u || n == 0u || n > (uint32_t)MB_N) {  // (workgroup-uniform)
        if (tid == 0) {
            o->n_out = 0u;
            o->flags = in_flags | RESULT_NEEDS_EXACT;
        }
        return;
    }
    const uint32_t n_sel = k < n ? k : n;
    if (n_sel >= 2u) {
        const uint32_t n_pairs = n * (n - 1u) / 2u;
        const uint32_t n_pass = (n_pairs + MB_THREADS - 1) / MB_THREADS;  // chains the busiest thread carries
        uint32_t pi[MB_PAIRS], pj[MB_PAIRS];
        Acc64<METRIC> A[MB_PAIRS];
#pragma unroll
        for (int c = 0; c < MB_PAIRS; ++c) {
            uint32_t rest = (uint32_t)tid + (uint32_t)c * MB_THREADS, i = 0;
            if (rest >= n_pairs) rest = 0;  // an idle chain computes pair (0, 1) and stores nothing
            while (rest >= n - 1u - i) {
                rest -= n - 1u - i;
                ++i;
            }
            pi[c] = i;
            pj[c] = i + 1u + rest;
            A[c].init();
        }
        // what this thread stages: slot -> (candidate, column); candidates >= n are clamped, never predicated
        const uint32_t n_stage = (n * MB_CH + MB_THREADS - 1) / MB_THREADS;  // slots below n * MB_CH, per thread
        uint64_t base[MB_PER];
#pragma unroll
        for (int e = 0; e < MB_PER; ++e) {
            uint32_t r = (uint32_t)(tid + e * MB_THREADS) / MB_CH;
            r = r < n ? r : n - 1u;
            uint32_t p = in->pos[r];
            p = p < index_rows ? p : 0u;  // a row is read from it; the host refuses such an answer
            base[e] = (uint64_t)p * dim;
        }
        double pre[MB_PER];
        auto fetch = [&](uint32_t c0) {
            const uint32_t cw = (dim - c0) < (uint32_t)MB_CH ? (dim - c0) : (uint32_t)MB_CH;
#pragma unroll
            for (int e = 0; e < MB_PER; ++e) {
                uint32_t cc = (uint32_t)(tid + e * MB_THREADS) % MB_CH;
                cc = cc < cw ? cc : cw - 1u;  // columns >= cw are never stepped
                if ((uint32_t)e < n_stage) pre[e] = master[base[e] + c0 + cc];
            }
        };
        const uint32_t n_chunks = (dim + MB_CH - 1) / MB_CH;
        if (n_chunks) fetch(0);
        for (uint32_t ch = 0; ch < n_chunks; ++ch) {
            const uint32_t c0 = ch * MB_CH;
            const uint32_t cw = (dim - c0) < (uint32_t)MB_CH ? (dim - c0) : (uint32_t)MB_CH;
            __syncthreads();  // the previous chunk's readers are done with the tile
#pragma unroll
            for (int e = 0; e < MB_PER; ++e) {
                const uint32_t s = (uint32_t)(tid + e * MB_THREADS);
                if ((uint32_t)e < n_stage) tile[s / MB_CH][s % MB_CH] = pre[e];
            }
            __syncthreads();
            if (ch + 1 < n_chunks) fetch(c0 + MB_CH);
#pragma unroll
            for (int c = 0; c < MB_PAIRS; ++c) {
                if ((uint32_t)c < n_pass) {
                    if (cw == (uint32_t)MB_CH) {
#pragma unroll
                        for (uint32_t cc = 0; cc < (uint32_t)MB_CH; ++cc) A[c].step(tile[pi[c]][cc], tile[pj[c]][cc]);
                    } else {
                        for (uint32_t cc = 0; cc < cw; ++cc) A[c].step(tile[pi[c]][cc], tile[pj[c]][cc]);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < MB_PAIRS; ++c) {
            if ((uint32_t)tid + (uint32_t)c * MB_THREADS < n_pairs) {
                const double s = A[c].score();
                sim[pi[c]][pj[c]] = s;
                sim[pj[c]][pi[c]] = s;  // the metrics are symmetric bit for bit
            }
        }
    }
    __syncthreads();
    if (tid >= WAVE) return;

    // the greedy selection, k_mmr_select's rounds in one wave
    const uint32_t i = (uint32_t)tid;
    const bool mine = i < n;
    const uint32_t my_pos = mine ? in->pos[i] : 0u;
    const double rel = mine ? in->score[i] : 0.0;
    double red = neg_inf<double>();
    asm volatile("" : "+v"(red));  // (TopList::init: keep the f64 -inf out of a scalar 64-bit literal)
    bool chosen = false;
    const double one_minus = __dsub_rn(1.0, lambda);
    if (i == 0u) {  // sel = [0]
        chosen = true;
        o->pos[0] = my_pos;
        o->score[0] = rel;
    }
    uint32_t last = 0u;
    for (uint32_t t = 1; t < n_sel; ++t) {
        double v = 0.0;
        uint32_t idx = POS_SENTINEL, first = POS_SENTINEL;
        if (mine && !chosen) {
            const double s = sim[last][i];
            if (s > red) red = s;  // a NaN similarity never replaces red
            v = __dsub_rn(__dmul_rn(lambda, rel), __dmul_rn(one_minus, red));
            first = (i << 1) | (v != v ? 1u : 0u);  // the smallest code = the first unselected candidate, bit 0: its v is NaN
            if (v == v) idx = i;                    // a NaN takes no part in the comparison
        }
#pragma unroll
        for (int w = 1; w < WAVE; w <<= 1) {
            const double ov = __shfl_xor(v, w);
            const uint32_t oidx = __shfl_xor(idx, w), ofirst = __shfl_xor(first, w);
            mmr_take_better(v, idx, ov, oidx);
            first = ofirst < first ? ofirst : first;
        }
        // the first unselected candidate stands unless a later comparison `v > v_best` succeeds: with a NaN there none does
        uint32_t best = idx;
        if (first != POS_SENTINEL && (first & 1u)) best = first >> 1;
        best = (uint32_t)__builtin_amdgcn_readfirstlane((int)best);
        if (best == POS_SENTINEL) break;  // (uniform; cannot happen while t < n)
        if (i == best) {
            chosen = true;
            o->pos[t] = my_pos;
            o->score[t] = rel;
        }
        last = best;
    }
    if (i == 0u) {  // the count and the flags last
        o->n_out = n_sel;
        o->flags = 0u;
    }
}

template <typename F>
hipError_t mmr_dispatch_metric(int metric, F&& f)
{
    switch (metric) {
    case COSINE: return f(std::integral_constant<int, COSINE>{});
    case EUCLIDEAN: return f(std::integral_constant<int, EUCLIDEAN>{});
    case MANHATTAN: return f(std::integral_constant<int, MANHATTAN>{});
    case DOT: return f(std::integral_constant<int, DOT>{});
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_mmr(hipStream_t s, int metric, const double* master, uint32_t dim, const MmrSource& src, double* sim,
                      uint32_t k, double lambda, SearchResultBlock* out, uint32_t seq)
{
    if (src.n == 0 || src.n > MMR_MAX_FETCH || k == 0 || !sim || !out || (!src.blocks && (!src.pos || !src.scores)))
        return hipErrorInvalidValue;
    const uint32_t tiles = (src.n + PW_T - 1) / PW_T;
    const uint32_t grid = tiles * (tiles + 1) / 2;
    hipError_t rc = hipSuccess;
    if (src.n >= 2 && k >= 2)  // one pick needs no similarity
        rc = mmr_dispatch_metric(metric, [&](auto M) -> hipError_t {
            hipLaunchKernelGGL((k_mmr_pairwise<decltype(M)::value>), dim3(grid), dim3(256), 0, s, master, dim, src, sim);
            return hipGetLastError();
        });
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(k_mmr_select, dim3(1), dim3(MMR_MAX_FETCH), 0, s, src, (const double*)sim, k, lambda, out, seq);
    return hipGetLastError();
}

hipError_t launch_mmr_batch(hipStream_t s, int metric, const Cand32* lists, const double* scores, int nq, const double* q_norms,
                            const double* master, uint32_t dim, uint64_t n_rows, uint64_t index_rows, uint32_t n_need, uint32_t k,
                            double lambda, double max_row_norm, double in_extra, SearchResultBlock* ranked, SearchResultBlock* out)
{
    if (nq <= 0 || !lists || !scores || !q_norms || !master || !ranked || !out || n_rows == 0 || n_need == 0 ||
        n_need > (uint32_t)MB_N || (uint64_t)n_need > n_rows || k == 0 || index_rows == 0 || index_rows >= 0xFFFFFFFFull ||
        metric == MANHATTAN)  // the MFMA filter's metrics: the batch has no Manhattan form
        return hipErrorInvalidValue;
    const uint32_t ld = (dim + 3u) & ~3u;
    return mmr_dispatch_metric(metric, [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        if constexpr (MM == MANHATTAN) {
            return hipErrorInvalidValue;
        } else {
            hipLaunchKernelGGL((k_mmr_batch_rank<MM>), dim3(((unsigned)nq + 3u) / 4u), dim3(256), 0, s, lists, scores, q_norms,
                               (uint32_t)nq, ld, n_rows, n_need, max_row_norm, in_extra, ranked);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((k_mmr_batch_select<MM>), dim3((unsigned)nq), dim3(MB_THREADS), 0, s, master, dim,
                               (uint32_t)index_rows, (const SearchResultBlock*)ranked, k, lambda, out);
            return hipGetLastError();
        }
    });
}

}  // namespace vl
