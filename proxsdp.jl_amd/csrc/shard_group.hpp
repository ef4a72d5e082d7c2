// In-process shard group: the meeting point of a block-sharded solve whose shards are host THREADS of one process
// (proxsdp_hip_solve_sharded).  GroupComm (shard_comm.hip.hpp) is the transport built on it; the callbacks and the RCCL
// communicator are the other two.  No HIP calls here: the group moves host records and publishes device pointers; the
// kernel that sums the coupling rows through those pointers is launched by GroupComm.
//
// barrier(): all shards meet, or the call throws.  It never hangs a caller: a shard that leaves the solve for any reason
// (leave(): an argument error in its sub-problem, a failed projection, an exception, or simply the end of its solve) wakes
// the waiting shards, and a barrier that can no longer complete throws PeerFailure; so does a wait longer than
// PROXSDP_HIP_COLLECTIVE_TIMEOUT_S seconds (default 300), after which the group stays abandoned.
//
// exchange(): every shard stores a record in its slot and all meet at ONE barrier; afterwards each shard reads all slots.
// The slots are double-buffered by the parity of the shard's call counter (all shards make the same sequence of calls): a
// shard overwrites slot [parity] at call k + 2, i.e. after the barrier of call k + 1, which every peer reaches only after
// it has finished reading call k's records.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace proxsdp {

// this shard stops because ANOTHER shard did (or never came): the secondary error of a group, never reported to the caller
// when some shard has an error of its own
struct PeerFailure : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// how long a shard waits for its peers in one collective, whatever the transport
inline double collective_timeout_s() {
    const char* e = std::getenv("PROXSDP_HIP_COLLECTIVE_TIMEOUT_S");
    return (e && std::atof(e) > 0.0) ? std::atof(e) : 300.0;
}

// The shards' packed records [sums | maxs] combined in rank order -- acc = rec(0); acc += rec(r) for r = 1, 2, ... and the
// element-wise std::max(acc, rec(r)) in the same order: sharded.make_reduce's order, the same bits on every shard.
// rec(r) points to shard r's record, wherever the transport keeps it.
template <typename Rec>
inline void combine_in_rank_order(Rec rec, int world, size_t ns, size_t nm, double* sums, double* maxs) {
    for (size_t q = 0; q < ns + nm; ++q) {
        double a = rec(0)[q];
        for (int r = 1; r < world; ++r) a = q < ns ? a + rec(r)[q] : std::max(a, rec(r)[q]);
        (q < ns ? sums[q] : maxs[q - ns]) = a;
    }
}

class ShardGroup {
public:
    explicit ShardGroup(int n_shards, double timeout_s = -1.0)
        : coup_part(2, std::vector<double*>(n_shards, nullptr)), device(n_shards, 0), S_(n_shards),
          timeout_s_(timeout_s > 0.0 ? timeout_s : collective_timeout_s()), calls_(n_shards, 0) {
        for (int par = 0; par < 2; ++par) rec_[par].resize(n_shards);
    }
    int size() const { return S_; }

    void barrier() {
        std::unique_lock<std::mutex> lk(mu_);
        if (abandoned_ || left_ > 0) throw PeerFailure(gone());
        const uint64_t g = gen_.load(std::memory_order_relaxed);
        if (++arrived_ == S_) {
            arrived_ = 0;
            gen_.store(g + 1, std::memory_order_release);
            cv_.notify_all();
            return;
        }
        // a short spin first (the peers run the same iteration: they are microseconds away), then sleep
        lk.unlock();
        for (int spin = 0; spin < 4000; ++spin) {
            if (gen_.load(std::memory_order_acquire) != g || stop_.load(std::memory_order_acquire)) break;
#if defined(__x86_64__)
            _mm_pause();
#endif
        }
        lk.lock();
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(timeout_s_);
        const bool ok = cv_.wait_until(lk, deadline, [&]() {
            return gen_.load(std::memory_order_relaxed) != g || abandoned_ || left_ > 0;
        });
        if (gen_.load(std::memory_order_relaxed) != g) return;          // the barrier completed (whatever happened since)
        if (!ok) {
            abandoned_ = true;
            stop_.store(true, std::memory_order_release);
            cv_.notify_all();
            throw PeerFailure("block-sharded solve: the shards did not meet within " + std::to_string((int)timeout_s_) +
                              " s (did another shard leave the solve?)");
        }
        throw PeerFailure(gone());
    }
    // this shard takes no further part: a barrier that waits for it, now or later, throws on the others
    void leave() {
        std::lock_guard<std::mutex> lk(mu_);
        ++left_;
        stop_.store(true, std::memory_order_release);
        cv_.notify_all();
    }

    // every shard has left.  Shards wait here before they free device memory that a peer's coupling-sum kernel may still be
    // reading.  NO deadline, on purpose: freeing under a running kernel is the worse outcome.  No barrier waits for ever, so
    // a shard that is gone always gets here; a shard that is HUNG inside a device call keeps the others waiting here -- the
    // collective timeout bounds the barriers, not this final join
    void wait_all_left() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&]() { return left_ >= S_; });
    }

    // store rec[0 .. n) as shard r's record of this call, meet, and return the parity under which all records are readable
    // (rec_[par][s]) until this shard's next-but-one call
    int exchange(int r, const double* rec, size_t n) {
        const int par = (int)(calls_[r]++ & 1);
        rec_[par][r].assign(rec, rec + n);
        barrier();
        for (int s = 0; s < S_; ++s)
            if (rec_[par][s].size() != n)
                throw std::logic_error("block-sharded solve: the shards' records differ in length (different call sequences)");
        return par;
    }

    // scalar reduce: the packed record [sums | maxs] of every shard, combined in shard order
    void reduce(int r, std::vector<double>& sums, std::vector<double>& maxs) {
        const size_t ns = sums.size(), nm = maxs.size();
        if (ns + nm == 0) return;
        std::vector<double> mine(sums);
        mine.insert(mine.end(), maxs.begin(), maxs.end());
        const int par = exchange(r, mine.data(), ns + nm);
        combine_in_rank_order([&](int s) { return rec_[par][s].data(); }, S_, ns, nm, sums.data(), maxs.data());
    }
    // element-wise sum of a host vector over the shards, in shard order (exit path: slacks of the coupling rows)
    void reduce_vec(int r, std::vector<double>& v) {
        const int par = exchange(r, v.data(), v.size());
        combine_in_rank_order([&](int s) { return rec_[par][s].data(); }, S_, v.size(), 0, v.data(), nullptr);
    }

    // coupling rows: coup_part[parity][s] = shard s's gathered partial buffer (device memory on device[s], or pinned host
    // memory when some pair of devices has no peer access: stage_host).  Written by shard s before its first coupling
    // barrier, read by every shard after it.
    std::vector<std::vector<double*>> coup_part;
    std::vector<int> device;
    bool stage_host = false;

private:
    std::string gone() const {
        return abandoned_ ? "block-sharded solve: the shard group was abandoned"
                          : "another shard of the block-sharded solve left the solve";
    }
    const int S_;
    const double timeout_s_;
    std::mutex mu_;
    std::condition_variable cv_;
    int arrived_ = 0, left_ = 0;
    bool abandoned_ = false;
    std::atomic<uint64_t> gen_{0};
    std::atomic<bool> stop_{false};
    std::vector<uint64_t> calls_;                         // per shard: exchange() calls so far (only shard r touches [r])
    std::vector<std::vector<double>> rec_[2];
};

}  // namespace proxsdp
