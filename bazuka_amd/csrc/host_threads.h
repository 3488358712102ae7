// Host threads for per-record work: how many a call may start, and the one task loop every host path runs its records through.  Plain C++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace bzk {

// Worker threads the host generator starts when the caller does not say: the CPUs this process may actually USE - the visible ones capped by the
// container's CPU quota (cgroup v2 cpu.max / v1 cfs quota).  The GPU pool's boxes show 256 CPUs under a 16-CPU quota: one thread per visible CPU
// there means 256 threads time-slicing 16 cores for a 256-transition witness (round 5, run 22: the deferred generator's bodies are short enough
// for that overhead to show in the CPU seconds).  Read once.
int host_default_threads();  // host_zk.hip

// fn(i) for every i < n on up to `threads` host threads (the caller's among them); returns when all have run
template <class F>
void host_for_each(uint64_t n, int threads, F fn) {
    std::atomic<uint64_t> next(0);
    auto worker = [&] {
        for (;;) {
            const uint64_t i = next.fetch_add(1);
            if (i >= n) break;
            fn(i);
        }
    };
    std::vector<std::thread> th;
    const int nt = (int)std::min<uint64_t>((uint64_t)std::max(threads, 1), n);
    for (int k = 1; k < nt; ++k) th.emplace_back(worker);
    worker();
    for (auto& x : th) x.join();
}

}  // namespace bzk
