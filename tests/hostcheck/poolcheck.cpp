// tests/hostcheck/poolcheck.cpp — TEST-ONLY driver for a ThreadSanitizer build (g++, CPU) of csrc/host_pool.h alone: the persistent host pool
// behind every batch verification, in the cases where its hand-written hand-over (generation counter, wanted / joined / running, two
// condition variables) can go wrong.  At most 8 threads.  Built and run by tests/test_sanitizers_host.py; prints "poolcheck ok" at the end,
// any ThreadSanitizer report fails the run.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "host_pool.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "poolcheck: check failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

using kzg_host::HostPool;

// job(i) adds i + 1 into slot i: afterwards every slot holds exactly i + 1 (ran once), whichever threads took part
static bool each_index_once(unsigned threads, size_t n) {
    std::vector<std::atomic<uint64_t>> slot(n);
    for (auto& s : slot) s.store(0);
    HostPool::get().run(threads, n, [&](size_t i) { slot[i].fetch_add(i + 1); });
    for (size_t i = 0; i < n; ++i) if (slot[i].load() != i + 1) return false;
    return true;
}

int main() {
    HostPool& pool = HostPool::get();
    // n = 0: the job is never called, with or without threads
    {
        std::atomic<int> calls{0};
        pool.run(8, 0, [&](size_t) { ++calls; });
        pool.run(1, 0, [&](size_t) { ++calls; });
        CHECK(calls.load() == 0);
    }
    CHECK(each_index_once(8, 1));                      // n = 1: the calling thread alone
    CHECK(each_index_once(8, 3));                      // n smaller than the thread count
    CHECK(each_index_once(1, 5));                      // one thread: serial
    CHECK(each_index_once(8, 1000));
    // the policy: never more threads than jobs, than the cap, or fewer than one; the exact override wins over the cap
    CHECK(kzg_host::host_threads(0, 8, 0) == 1 && kzg_host::host_threads(3, 8, 0) <= 3 && kzg_host::host_threads(1000, 8, 0) <= 8);
    CHECK(kzg_host::host_threads(1000, 8, 5) == 5 && kzg_host::host_threads(2, 8, 5) == 2);
    CHECK(kzg_host::host_threads_cap(8) == 8 && kzg_host::host_threads_cap(0) >= 2 && kzg_host::host_threads_cap(0) <= 48 && kzg_host::host_threads_cap(1000) <= 48);
    // back-to-back runs with alternating thread counts: late wakers of an old generation meet a run that wants fewer threads
    {
        const unsigned counts[3] = {2, 8, 3};
        for (int rep = 0; rep < 200; ++rep) CHECK(each_index_once(counts[rep % 3], 64 + (size_t)rep));
    }
    // two caller threads at once: the runs take turns, each sees only its own jobs
    {
        std::atomic<int> bad{0};
        auto caller = [&](unsigned threads) { for (int rep = 0; rep < 50; ++rep) if (!each_index_once(threads, 200)) ++bad; };
        std::thread a(caller, 8u), b(caller, 4u);
        a.join(); b.join();
        CHECK(bad.load() == 0);
    }
    printf("poolcheck ok\n");
    return 0;
}
