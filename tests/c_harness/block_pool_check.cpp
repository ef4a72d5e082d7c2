// Stand-alone check of csrc/block_pool.hpp (host-only, no HIP): BlockPool::run from pools of 1, 2 and 8 threads -- every
// index of a call runs exactly once, after its thread's init; a throwing job's first error is rethrown once the other jobs
// of the call have run, and the next call works; the pool is destroyed with idle workers.  Meant for the sanitizers:
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=thread            -I proxsdp.jl_amd/csrc tests/c_harness/block_pool_check.cpp
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -I proxsdp.jl_amd/csrc tests/c_harness/block_pool_check.cpp
// Exit status 0 and "ok" on success.
#include <atomic>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "block_pool.hpp"

namespace {
thread_local bool t_init = false;

int check(int nthreads) {
    int bad = 0;
    std::atomic<int> inits{0};
    {
        proxsdp::BlockPool pool(nthreads, [&inits]() { t_init = true; ++inits; });
        std::vector<std::atomic<int>> hits(64);
        std::atomic<int> no_init{0};
        for (int call = 0; call < 600; ++call) {
            const int cnt = 1 + (call * 7) % 64;                   // 1 .. 64 indices, not in order
            std::vector<int> idx(cnt);
            for (int q = 0; q < cnt; ++q) idx[q] = (q * 37 + call) % 64;        // (37 is coprime to 64: distinct)
            for (auto& h : hits) h = 0;
            // every 5th call: two jobs throw; one pool thread takes the indices in the order listed, so there the first
            // listed thrower's error is the one that comes back
            const bool throws = call % 5 == 3 && cnt >= 2;
            const int bad_a = idx[0], bad_b = idx[cnt - 1];
            std::string got;
            try {
                pool.run(idx, [&](int i) {
                    if (!t_init) ++no_init;
                    ++hits[i];
                    if (throws && (i == bad_a || i == bad_b)) throw std::runtime_error(std::to_string(i));
                });
            } catch (const std::runtime_error& e) { got = e.what(); }
            if (throws) {
                bad += got != std::to_string(bad_a) && got != std::to_string(bad_b);
                if (nthreads == 1) bad += got != std::to_string(bad_a);
            } else {
                bad += !got.empty();
            }
            std::vector<int> want(64, 0);
            for (int i : idx) want[i] = 1;
            for (int i = 0; i < 64; ++i) bad += hits[i] != want[i];             // once each, the throwing call's too
        }
        bad += no_init != 0;
        pool.run({}, [&](int) { ++bad; });                          // nothing listed: nothing runs
    }                                                               // (destroyed with idle workers)
    bad += inits != nthreads;
    { proxsdp::BlockPool unused(nthreads, []() {}); }               // ... and one that never ran a job
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    for (int nthreads : {1, 2, 8}) {
        bad += check(nthreads);
        std::printf("threads = %d: %s\n", nthreads, bad ? "FAILED" : "ok");
    }
    return bad ? 1 : 0;
}
