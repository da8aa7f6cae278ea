// Unit test of the TopList machinery on hardware (debug tool, not shipped): insert / offer, and the two steps of the f32
// batch scan's lazy insertion, sort64_reversed and TopList::merge_reversed, against std::stable_sort on (key desc, pos asc).
#include "../../vectorlite_amd/csrc/kernels.hip"
#include <cstdio>
#include <vector>
#include <algorithm>
#include <random>
#include <limits>
using namespace vl;
template <typename K>
__global__ void k_offer(const K* keys, const uint32_t* pos, int n, int active_per_step, K* out_k, uint32_t* out_p)
{
    TopList<K> L; L.init();
    int lane = threadIdx.x;
    for (int s = 0; s < n; s += 64) {
        int i = s + lane;
        bool valid = i < n && lane < active_per_step;
        K k = valid ? keys[i] : (K)0;
        L.offer(k, valid ? pos[i] : 0u, valid);
    }
    out_k[lane] = L.key; out_p[lane] = L.pos;
}
template <typename K>
int run(int n, int active, int seed, int mode)
{
    std::mt19937 rng(seed);
    std::vector<K> keys(n); std::vector<uint32_t> pos(n);
    for (int i = 0; i < n; ++i) { pos[i] = i; keys[i] = mode == 0 ? (K)((rng() & 1) ? 1.0 : -1.0) : (K)((int)(rng() % 1000) - 500) / (K)7; }
    K* dk; uint32_t* dp; K* ok; uint32_t* op;
    (void)hipMalloc(&dk, n * sizeof(K)); (void)hipMalloc(&dp, n * 4); (void)hipMalloc(&ok, 64 * sizeof(K)); (void)hipMalloc(&op, 64 * 4);
    (void)hipMemcpy(dk, keys.data(), n * sizeof(K), hipMemcpyHostToDevice); (void)hipMemcpy(dp, pos.data(), n * 4, hipMemcpyHostToDevice);
    k_offer<K><<<1, 64>>>(dk, dp, n, active, ok, op);
    std::vector<K> hk(64); std::vector<uint32_t> hp(64);
    (void)hipMemcpy(hk.data(), ok, 64 * sizeof(K), hipMemcpyDeviceToHost); (void)hipMemcpy(hp.data(), op, 64 * 4, hipMemcpyDeviceToHost);
    std::vector<int> idx;
    for (int s = 0; s < n; s += 64) for (int l = 0; l < 64 && s + l < n; ++l) if (l < active) idx.push_back(s + l);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return keys[a] > keys[b] || (keys[a] == keys[b] && pos[a] < pos[b]); });
    int bad = 0;
    for (int i = 0; i < 64; ++i) {
        uint32_t wp = i < (int)idx.size() ? pos[idx[i]] : 0xFFFFFFFFu;
        if (hp[i] != wp) { if (bad < 3) printf("  n=%d active=%d mode=%d lane %d got pos %u key %g want pos %u\n", n, active, mode, i, hp[i], (double)hk[i], wp); bad++; }
    }
    (void)hipFree(dk); (void)hipFree(dp); (void)hipFree(ok); (void)hipFree(op);
    return bad;
}

// ---- sort64_reversed and TopList::merge_reversed: the two steps of k_scan_batch's buffer flush ----
constexpr uint32_t SENT = 0xFFFFFFFFu;
template <typename K>
struct Ent {
    K key;
    uint32_t pos;
};
template <typename K>
bool ent_better(const Ent<K>& a, const Ent<K>& b) { return a.key > b.key || (a.key == b.key && a.pos < b.pos); }
template <typename K>
Ent<K> filler() { return Ent<K>{-std::numeric_limits<K>::infinity(), SENT}; }
// mode 0: two key values, 1: many values with some ties, 2: every key equal
template <typename K>
K test_key(std::mt19937& rng, int mode) { return mode == 0 ? (K)((rng() & 1) ? 1.0 : -1.0) : mode == 1 ? (K)((int)(rng() % 1000) - 500) / (K)7 : (K)0.25; }

template <typename K>
__global__ void k_sort_reversed(const Ent<K>* in, Ent<K>* out)
{
    const int lane = threadIdx.x;
    K k = in[lane].key;
    uint32_t p = in[lane].pos;
    sort64_reversed<K>(k, p);
    out[lane].key = k;
    out[lane].pos = p;
}
// list[64] sorted best-first (fillers last); buf[64]: sorted best-first and read reversed, or (do_sort) in any order and
// sorted by sort64_reversed first, as the flush does.  out[64] = the merged list, out[64] = (thr_key, thr_pos).
template <typename K>
__global__ void k_merge_reversed(const Ent<K>* list, const Ent<K>* buf, int do_sort, Ent<K>* out)
{
    const int lane = threadIdx.x;
    TopList<K> L;
    L.init();
    L.key = list[lane].key;
    L.pos = list[lane].pos;
    Ent<K> e = buf[do_sort ? lane : 63 - lane];
    if (do_sort) sort64_reversed<K>(e.key, e.pos);
    L.merge_reversed(e.key, e.pos);
    out[lane].key = L.key;
    out[lane].pos = L.pos;
    if (lane == 0) {
        out[64].key = L.thr_key;
        out[64].pos = L.thr_pos;
    }
}
template <typename K>
struct DevBuf {
    Ent<K>* p = nullptr;
    explicit DevBuf(int count) { (void)hipMalloc(&p, count * sizeof(Ent<K>)); (void)hipMemset(p, 0, count * sizeof(Ent<K>)); }
    ~DevBuf() { (void)hipFree(p); }
    void put(const std::vector<Ent<K>>& v) { (void)hipMemcpy(p, v.data(), v.size() * sizeof(Ent<K>), hipMemcpyHostToDevice); }
    std::vector<Ent<K>> get(int count) { std::vector<Ent<K>> v(count); (void)hipMemcpy(v.data(), p, count * sizeof(Ent<K>), hipMemcpyDeviceToHost); return v; }
};
// `count` entries with distinct shuffled positions taken from pool[first ..), padded to 64 with fillers
template <typename K>
std::vector<Ent<K>> make_entries(std::mt19937& rng, const std::vector<uint32_t>& pool, int first, int count, int mode)
{
    std::vector<Ent<K>> v(64, filler<K>());
    for (int i = 0; i < count; ++i) v[i] = Ent<K>{test_key<K>(rng, mode), pool[first + i]};
    return v;
}
template <typename K>
int run_sort(int filled, int seed, int mode)
{
    std::mt19937 rng(seed);
    std::vector<uint32_t> pool(1000);
    for (int i = 0; i < 1000; ++i) pool[i] = i;
    std::shuffle(pool.begin(), pool.end(), rng);
    std::vector<Ent<K>> in = make_entries<K>(rng, pool, 0, filled, mode);
    DevBuf<K> di(64), dout(64);
    di.put(in);
    k_sort_reversed<K><<<1, 64>>>(di.p, dout.p);
    std::vector<Ent<K>> got = dout.get(64);
    std::stable_sort(in.begin(), in.end(), ent_better<K>);
    int bad = 0;
    for (int i = 0; i < 64; ++i) {
        const Ent<K>& w = in[63 - i];
        if (!(got[i].key == w.key) || got[i].pos != w.pos) { if (bad < 3) printf("  sort filled=%d mode=%d lane %d got (%g, %u) want (%g, %u)\n", filled, mode, i, (double)got[i].key, got[i].pos, (double)w.key, w.pos); bad++; }
    }
    return bad;
}
template <typename K>
int run_merge(int in_list, int in_buf, int seed, int mode, int do_sort)
{
    std::mt19937 rng(seed);
    std::vector<uint32_t> pool(1000);
    for (int i = 0; i < 1000; ++i) pool[i] = i;
    std::shuffle(pool.begin(), pool.end(), rng);
    std::vector<Ent<K>> list = make_entries<K>(rng, pool, 0, in_list, mode), buf = make_entries<K>(rng, pool, 64, in_buf, mode);
    std::stable_sort(list.begin(), list.end(), ent_better<K>);
    if (!do_sort) std::stable_sort(buf.begin(), buf.end(), ent_better<K>);
    DevBuf<K> dl(64), db(64), dout(65);
    dl.put(list);
    db.put(buf);
    k_merge_reversed<K><<<1, 64>>>(dl.p, db.p, do_sort, dout.p);
    std::vector<Ent<K>> got = dout.get(65);
    std::vector<Ent<K>> all(list);
    all.insert(all.end(), buf.begin(), buf.end());
    std::stable_sort(all.begin(), all.end(), ent_better<K>);  // the 64 best of the union; ties at the cut go to the lower position
    int bad = 0;
    for (int i = 0; i < 65; ++i) {
        const Ent<K>& w = all[i < 64 ? i : 63];  // entry 64: the threshold copy of the 64th place
        if (!(got[i].key == w.key) || got[i].pos != w.pos) { if (bad < 3) printf("  merge list=%d buf=%d mode=%d sort=%d lane %d got (%g, %u) want (%g, %u)\n", in_list, in_buf, mode, do_sort, i, (double)got[i].key, got[i].pos, (double)w.key, w.pos); bad++; }
    }
    return bad;
}

int main()
{
    int total = 0;
    for (int mode = 0; mode < 3; ++mode) {
        for (int filled : {64, 1, 60, 63, 0}) {
            int a = run_sort<float>(filled, 100 * mode + filled, mode);
            int b = run_sort<double>(filled, 100 * mode + filled, mode);
            if (a || b) printf("sort64_reversed filled=%d mode=%d: float bad=%d double bad=%d\n", filled, mode, a, b);
            total += a + b;
        }
        // a list that is empty, half full or full takes a buffer of 1, 33, 60 or 64 entries; modes 0 and 2 tie across the 64th place
        for (int in_list : {0, 32, 64})
            for (int in_buf : {1, 33, 60, 64})
                for (int do_sort = 0; do_sort < 2; ++do_sort) {
                    int a = run_merge<float>(in_list, in_buf, 1000 * mode + 70 * in_list + in_buf, mode, do_sort);
                    int b = run_merge<double>(in_list, in_buf, 1000 * mode + 70 * in_list + in_buf, mode, do_sort);
                    if (a || b) printf("merge_reversed list=%d buf=%d mode=%d sort=%d: float bad=%d double bad=%d\n", in_list, in_buf, mode, do_sort, a, b);
                    total += a + b;
                }
    }
    for (int mode = 0; mode < 2; ++mode)
        for (int n : {1, 5, 64, 65, 128, 1000})
            for (int active : {64, 1, 33}) {
                int a = run<float>(n, active, n * 7 + active, mode);
                int b = run<double>(n, active, n * 7 + active, mode);
                if (a || b) printf("n=%d active=%d mode=%d: float bad=%d double bad=%d\n", n, active, mode, a, b);
                total += a + b;
            }
    printf("total bad %d\n", total);
    return 0;
}
