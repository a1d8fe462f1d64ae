// host_pool.h — the library's persistent pool of host threads and the policy that sizes it.  The pool carries the host side of batch
// verification: the Fiat-Shamir transcripts, the point validation, the scalars of the linear combinations, the two Miller loops.
// Pure host code (no HIP, no engine.h): also compiled alone by g++ under ThreadSanitizer (tests/hostcheck/poolcheck.cpp).  The two
// overrides of the policy (KZG_HOST_THREADS_MAX, KZG_HOST_THREADS) come from the caller: runtime.hip passes them from opts().
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <pthread.h>
#include <thread>
#include <vector>

namespace kzg_host {

// CPUs this process may use on average: the CFS bandwidth quota of its cgroup (v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us), 0 = none.
// A pool wider than the quota allows runs fine for one call, but back-to-back calls then spend the period's budget early and the kernel
// freezes EVERY thread of the cgroup until the next 100 ms period: that was the 20-34 ms tail of batch verification (1 call in 9; DESIGN.md
// section 6, profiles/r06_batch_verify_tail.md: every slow call coincides with a throttled period in cpu.stat, none without).
inline double cgroup_cpu_quota() {
    static const double q = []() -> double {
        auto read2 = [](const char* path, char a[64], char b[64]) {
            FILE* f = fopen(path, "r");
            if (!f) return 0;
            const int got = fscanf(f, "%63s %63s", a, b);
            fclose(f);
            return got;
        };
        char a[64] = {0}, b[64] = {0};
        if (read2("/sys/fs/cgroup/cpu.max", a, b) == 2 && strcmp(a, "max") != 0 && atof(b) > 0) return atof(a) / atof(b);
        char c[64] = {0}, d[64] = {0};
        if (read2("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", a, b) >= 1 && read2("/sys/fs/cgroup/cpu/cpu.cfs_period_us", c, d) >= 1 && atof(a) > 0 && atof(c) > 0)
            return atof(a) / atof(c);
        return 0.0;
    }();
    return q;
}
// Upper bound of the pool, whatever the core count.  Measured on the 256-thread host of an MI355X box, 4 096-row batch verification
// end to end (tools/trace_batch_verify.py): 32 threads 6.3-6.5 ms, 48 5.4-5.5, 64 5.3-5.6, 96 5.8-5.9, 128 6.0-6.5 (the transcripts scale, the upload and the
// serial parts do not, and past 64 the pool's wake-ups cost more than they gain) -> 48.
// 48 threads at most; under a CPU quota of Q, Q threads: the pool then never draws more than the quota, whatever else the process runs (HIP's
// helper threads, the caller's own).  Measured on a 16-CPU quota, 4 096 blobs per call, 60 calls each: 48 threads median 6.2 ms / max 24 / 123 ms of CPU per
// call; 32: 6.1 / 15 / 109; 24: 6.8 / 7.2 / 100; 20: 6.9 / 7.0 / 88 (but 13.7 once in 40 calls inside bench.py); 16: 7.7 / 7.8 / 84; 12: 9.4 / 9.8 / 86.
// max_override (KZG_HOST_THREADS_MAX) in [1, 256] replaces the whole rule.
inline unsigned host_threads_cap(int max_override) {
    if (max_override >= 1 && max_override <= 256) return (unsigned)max_override;
    unsigned c = 48;
    const double q = cgroup_cpu_quota();
    if (q > 0) c = std::min<unsigned>(c, std::max<unsigned>(2u, (unsigned)q));
    return c;
}
// threads (the calling one included) for `jobs` jobs under that cap; exact_override (KZG_HOST_THREADS) > 0: exactly that many (measurements)
inline unsigned host_threads(size_t jobs, unsigned cap, int exact_override) {
    unsigned t = std::thread::hardware_concurrency();
    if (t == 0) t = 4;
    if (t > cap) t = cap;
    if (exact_override > 0) t = (unsigned)exact_override;
    if ((size_t)t > jobs) t = (unsigned)jobs;
    return t ? t : 1;
}

// A persistent pool of host threads (created on first use, parked on a condition variable between calls; a parked worker wakes in
// ~20 us): spawning 31 threads per call cost 0.3-1 ms, three times per batch verification.  run(T, n, job) executes job(i) for i in
// [0, n) on T - 1 pool threads AND the calling thread; one run at a time.
class HostPool {
public:
    static HostPool& get() { static HostPool pool; return pool; }
    void run(unsigned T, size_t n, const std::function<void(size_t)>& job) {
        if (n == 0) return;
        if ((size_t)T > n) T = (unsigned)n;
        if (T <= 1) { for (size_t i = 0; i < n; ++i) job(i); return; }
        std::lock_guard<std::mutex> one(run_mu_);
        ensure(T - 1);
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &job; n_ = n; next_.store(0, std::memory_order_relaxed);
            wanted_ = T - 1; joined_ = 0; running_ = 0;
            ++generation_;
        }
        cv_work_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(mu_);
        wanted_ = 0;                                               // late wakers of this generation find nothing to join
        cv_done_.wait(lk, [&] { return running_ == 0; });
        job_ = nullptr;
    }
private:
    HostPool() = default;
    ~HostPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_work_.notify_all();
        for (auto& t : threads_) t.join();
    }
    void ensure(unsigned count) {
        while (threads_.size() < count)
            threads_.emplace_back([this] { pthread_setname_np(pthread_self(), "kzg-pool"); loop(); });     // visible in /proc/<pid>/task/*/comm (tools/trace_batch_verify.py)
    }
    void work() { for (;;) { const size_t i = next_.fetch_add(1, std::memory_order_relaxed); if (i >= n_) return; (*job_)(i); } }
    void loop() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_work_.wait(lk, [&] { return stop_ || generation_ != seen; });
            if (stop_) return;
            seen = generation_;
            if (joined_ >= wanted_) continue;                      // this run wants fewer threads than the pool has
            ++joined_; ++running_;
            lk.unlock();
            work();
            lk.lock();
            if (--running_ == 0) cv_done_.notify_all();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_, run_mu_;
    std::condition_variable cv_work_, cv_done_;
    const std::function<void(size_t)>* job_ = nullptr;
    size_t n_ = 0;
    std::atomic<size_t> next_{0};
    unsigned wanted_ = 0, joined_ = 0, running_ = 0;
    uint64_t generation_ = 0;
    bool stop_ = false;
};

}  // namespace kzg_host
