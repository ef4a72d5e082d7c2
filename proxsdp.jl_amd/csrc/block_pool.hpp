// Job pool of the concurrent block projections (host only: no HIP in this header).
//
// A fixed set of sleeping worker threads; run(indices, job) hands job(index) out for every listed index and blocks until
// all of them are done.  The jobs are long (one PSD block's projection: many launches and read-backs), so the workers wait
// on a condition variable -- unlike SpinPool (host_util.hpp), whose jobs are shorter than a wake-up.
#pragma once
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace proxsdp {

class BlockPool {
public:
    // init() runs once on every worker thread before its first job (the solver selects its device there); it must not throw
    BlockPool(int nthreads, std::function<void()> init) {
        try {
            for (int t = 0; t < nthreads; ++t)
                workers_.emplace_back([this, init]() { init(); loop(); });
        } catch (...) {                        // a thread could not be started: the ones that were are joined, not abandoned
            stop_and_join();
            throw;
        }
    }
    ~BlockPool() { stop_and_join(); }
    BlockPool(const BlockPool&) = delete;
    BlockPool& operator=(const BlockPool&) = delete;
    // job(idx) for every listed index, on the workers; the indices are taken in the order listed.  Returns when every job
    // is done; the first exception a job threw is rethrown then (the other jobs of the call still ran), and the pool
    // serves the next call as before.  One caller at a time.
    void run(const std::vector<int>& indices, const std::function<void(int)>& job) {
        if (indices.empty()) return;
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &job;
            queue_.assign(indices.rbegin(), indices.rend());
            pending_ = (int)indices.size();
            error_ = nullptr;
        }
        cv_.notify_all();
        std::exception_ptr err;
        {
            std::unique_lock<std::mutex> lk(mu_);
            done_cv_.wait(lk, [this]() { return pending_ == 0; });
            err = error_;
            error_ = nullptr;
            job_ = nullptr;
        }
        if (err) std::rethrow_exception(err);
    }

private:
    void stop_and_join() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread& t : workers_) if (t.joinable()) t.join();
    }
    void loop() {
        for (;;) {
            int idx;
            const std::function<void(int)>* job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this]() { return stop_ || !queue_.empty(); });
                if (stop_) return;
                idx = queue_.back();
                queue_.pop_back();
                job = job_;
            }
            try {
                (*job)(idx);
            } catch (...) {
                std::lock_guard<std::mutex> lk(mu_);
                if (!error_) error_ = std::current_exception();
            }
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (--pending_ == 0) done_cv_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<int> queue_;                   // indices waiting for a worker, last one first
    int pending_ = 0;
    bool stop_ = false;
    std::exception_ptr error_;
    const std::function<void(int)>* job_ = nullptr;
};

}  // namespace proxsdp
