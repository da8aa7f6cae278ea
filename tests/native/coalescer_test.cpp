// CPU unit test of csrc/coalescer.hpp (header-only, no HIP): a pass that THROWS must still release every caller --
// followers already taken off the queue are marked done, the leader slot is freed, later callers become leaders.
// Built and run by tests/test_coalescer_cpu.py with g++ -pthread.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../vectorlite_amd/csrc/coalescer.hpp"

struct Req {
    int id;
    int rc = 6;  // "unanswered" until a pass sets it
    bool done = false;
};

// Adaptive gather (window 0): 8 callers in a closed loop on 2 ms passes.  Without it the passes alternate 1 / 7 (the first
// caller back leads alone while the others are returning): ~2 passes per round.  With it the leader waits (<= a quarter of the
// pass time) for as many requests as the last passes held: ~1 pass per round.  A lone caller never waits.
// The callers start together: each one waits at a gate until all of them exist (creating a thread is slow under the
// sanitizers, and callers that start while others are still being created fill the first passes only partly).  *ms, if
// given, is the time from the gate's opening to the last caller's return.
static int closed_loop(bool adaptive, int threads, int rounds, uint64_t* passes, uint64_t* waits, double* ms = nullptr)
{
    vl::Coalescer<Req> co;
    co.configure(64, 0, 1024);
    co.set_adaptive(adaptive);
    auto same = [](const Req&, const Req&) { return true; };
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    std::mutex gate_mu;
    std::condition_variable gate_cv;
    int ready = 0;
    bool open = false;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            {
                std::unique_lock<std::mutex> g(gate_mu);
                if (++ready == threads) gate_cv.notify_all();
                gate_cv.wait(g, [&] { return open; });
            }
            for (int i = 0; i < rounds; ++i) {
                Req r{t * 1000 + i};
                co.run(r, same, [&](std::vector<Req*>& batch) {
                    std::this_thread::sleep_for(std::chrono::milliseconds(2));
                    for (Req* o : batch) o->rc = 0;
                });
                if (!r.done || r.rc != 0) bad.fetch_add(1);
            }
        });
    std::chrono::steady_clock::time_point t0;
    {
        std::unique_lock<std::mutex> g(gate_mu);
        gate_cv.wait(g, [&] { return ready == threads; });
        open = true;
        t0 = std::chrono::steady_clock::now();
    }
    gate_cv.notify_all();
    for (auto& t : th) t.join();
    if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    uint64_t q = 0, us = 0;
    co.stats(passes, &q);
    co.gather_stats(waits, &us);
    return bad.load() == 0 && q == (uint64_t)threads * rounds ? 0 : 1;
}

static int adaptive_gather()
{
    uint64_t p_off = 0, w_off = 0, p_on = 0, w_on = 0, p_lone = 0, w_lone = 0;
    if (closed_loop(false, 8, 25, &p_off, &w_off)) return 10;
    if (closed_loop(true, 8, 25, &p_on, &w_on)) return 11;
    if (closed_loop(true, 1, 25, &p_lone, &w_lone)) return 12;
    std::printf("closed loop, 8 callers x 25 rounds: %llu passes without the gather, %llu with it (%llu waits); lone caller: %llu passes, %llu waits\n",
                (unsigned long long)p_off, (unsigned long long)p_on, (unsigned long long)w_on, (unsigned long long)p_lone,
                (unsigned long long)w_lone);
    if (w_off != 0 || w_lone != 0 || p_lone != 25) return 13;  // no waiting when it is off, none for a lone caller
    if (p_on > 34) return 14;                                  // ~25 passes of 8 (a few smaller ones while it settles)
    // many callers on few cores: arrivals wake the gathering leader only, so 200 callers x 6 rounds of 2 ms passes finish in
    // about 6 passes' time (a wake-up of every sleeper per arrival used to take tens of milliseconds per pass)
    uint64_t p_many = 0, w_many = 0;
    double ms = 0.0;
    if (closed_loop(true, 200, 6, &p_many, &w_many, &ms)) return 15;
    std::printf("200 callers x 6 rounds: %llu passes, %.1f ms\n", (unsigned long long)p_many, ms);
    if (p_many > 30 || ms > 400.0) return 16;
    return 0;
}

int main()
{
    vl::Coalescer<Req> co;
    co.configure(64, 2000, 1024);  // a 2 ms window so that callers pile up behind the first leader
    std::atomic<int> passes{0}, answered{0}, unanswered{0};
    auto same = [](const Req&, const Req&) { return true; };
    auto worker = [&](int id) {
        Req r{id};
        co.run(r, same, [&](std::vector<Req*>& batch) {
            const int p = passes.fetch_add(1);
            if (p == 0) {  // the first pass answers half of its batch, then dies
                for (size_t i = 0; i < batch.size() / 2; ++i) batch[i]->rc = 0;
                throw std::length_error("k = u64::MAX");
            }
            for (Req* o : batch) o->rc = 0;
        });
        if (!r.done) std::abort();
        (r.rc == 0 ? answered : unanswered).fetch_add(1);
    };
    std::vector<std::thread> th;
    for (int i = 0; i < 24; ++i) th.emplace_back(worker, i);
    // every thread must come back: a deadlocked coalescer hangs here and the pytest timeout reports it
    for (auto& t : th) t.join();
    // after the failed pass the coalescer still works
    for (int i = 0; i < 4; ++i) worker(100 + i);
    uint64_t b = 0, q = 0;
    co.stats(&b, &q);
    std::printf("passes %d answered %d unanswered %d stats %llu/%llu\n", passes.load(), answered.load(), unanswered.load(),
                (unsigned long long)b, (unsigned long long)q);
    if (answered.load() + unanswered.load() != 28) return 2;
    if (unanswered.load() > 24) return 3;  // requests the dead pass left unanswered keep their error rc: reported, not hung
    return adaptive_gather();
}
