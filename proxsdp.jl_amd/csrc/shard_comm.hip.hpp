// The transport of a block-sharded solve: what the PDHG loop asks of "the other shards", and the three ways to serve it.
//   CallbackComm -- the caller's reduce_fn / reduce_vec_fn (gloo, torch-NCCL)
//   RcclComm     -- the library's own RCCL calls on the solver's stream (proxsdp_problem.nccl_comm, rccl_dl.hpp)
//   GroupComm    -- shards that are host threads of one process (proxsdp_hip_solve_sharded, shard_group.hpp)
// Solver holds one ShardComm (none when the solve is not sharded); a ShardComm sees the stream it is to work on, the
// statistics record and options.host_wait_spin, never the solver.  Included by solver.hip.hpp below DevBuf and poll_ready.
#pragma once

namespace proxsdp {

// wait for a stream at a read-back on the critical path: spinning on the query, or blocked in the runtime
inline void wait_for_stream(hipStream_t s, bool spin) {
    if (spin) poll_ready([&]() { return hipStreamQuery(s); }, []() {});
    else PX_HIP(hipStreamSynchronize(s));
}
// v[rows[k]] <- sum over the shards of tab[s][k]: the in-process group's coupling sum (also proxsdp_hip_coupling_sum)
inline void launch_coupling_sum(hipStream_t s, const double* const* tab, int nshard, const int* rows, int cnt, double* v) {
    hipLaunchKernelGGL(dev::k_coupling_sum, dim3(ceil_div(cnt, dev::TPB)), dim3(dev::TPB), 0, s, tab, nshard, rows, cnt, v);
}

class ShardComm {
public:
    virtual ~ShardComm() = default;
    // scalar reduce: sums added in rank order, maxs element-wise -- the same bits on every shard
    virtual void reduce(hipStream_t s, std::vector<double>& sums, std::vector<double>& maxs) = 0;
    // element-wise sum of a host vector (exit path: slacks of the coupling rows)
    virtual void reduce_vec_host(hipStream_t s, std::vector<double>& v) = 0;
    virtual void setup_coupling(size_t nc, hipStream_t s) = 0;       // buffers that depend on the number of coupling rows
    // Mx[rows] <- sum over the shards: gathered into the transport's buffer, summed there or through it
    void reduce_coupling(hipStream_t s, double* Mx_dev, const int* rows_d, int nc) {
        hipLaunchKernelGGL(dev::k_gather_rows, dim3(ceil_div(nc, dev::TPB)), dim3(dev::TPB), 0, s,
                           (const double*)Mx_dev, rows_d, nc, next_gather_buffer());
        sum_gathered(s, Mx_dev, rows_d, nc);
    }
    // a host wait on s that may sit behind a collective: true when the transport waited, within its own bound
    virtual bool bounded_wait(hipStream_t) { return false; }
    // the solve is failing: stop a collective of it that may be pending; true when the caller's communicator was aborted
    virtual bool abort_if_pending() { return false; }

protected:
    virtual double* next_gather_buffer() = 0;
    virtual void sum_gathered(hipStream_t s, double* Mx_dev, const int* rows_d, int nc) = 0;
    static void scatter(hipStream_t s, double* Mx_dev, const int* rows_d, int nc, const double* buf) {
        hipLaunchKernelGGL(dev::k_scatter_rows, dim3(ceil_div(nc, dev::TPB)), dim3(dev::TPB), 0, s, Mx_dev, rows_d, nc, buf);
    }
};

// the caller's callbacks (include/proxsdp_hip.h): the coupling rows go through the CALLER's stream or through host memory
class CallbackComm : public ShardComm {
    int (*reduce_fn)(void*, double*, int32_t, double*, int32_t);
    int (*reduce_vec_fn)(void*, double*, int64_t, int32_t);
    void* ctx;
    bool on_device;
    DevBuf<double> buf;
    std::vector<double> host;
    double* next_gather_buffer() override { return buf.p; }
    void sum_gathered(hipStream_t s, double* Mx_dev, const int* rows_d, int nc) override {
        if (on_device) {
            PX_HIP(hipStreamSynchronize(s));                 // the collective runs on the caller's stream
            if (reduce_vec_fn(ctx, buf.p, nc, 1) != 0) throw std::runtime_error("reduce_vec_fn failed");
        } else {
            host.resize(nc);
            buf.download(host.data(), nc, s);
            PX_HIP(hipStreamSynchronize(s));
            reduce_vec_host(s, host);
            buf.upload(host.data(), nc, s);
        }
        scatter(s, Mx_dev, rows_d, nc, buf.p);
    }

public:
    explicit CallbackComm(const proxsdp_problem& prob)
        : reduce_fn(prob.reduce_fn), reduce_vec_fn(prob.reduce_vec_fn), ctx(prob.reduce_ctx), on_device(prob.reduce_vec_on_device != 0) {}
    void reduce(hipStream_t, std::vector<double>& sums, std::vector<double>& maxs) override {
        if (reduce_fn(ctx, sums.data(), (int32_t)sums.size(), maxs.data(), (int32_t)maxs.size()) != 0)
            throw std::runtime_error("reduce_fn failed");
    }
    void reduce_vec_host(hipStream_t, std::vector<double>& v) override {
        if (reduce_vec_fn(ctx, v.data(), (int64_t)v.size(), 0) != 0) throw std::runtime_error("reduce_vec_fn failed");
    }
    void setup_coupling(size_t nc, hipStream_t) override { buf.alloc(nc); }
};

// Native RCCL: one all-gather of the packed scalar record per reduce (<= 400 bytes per rank: latency-bound over xGMI),
// combined on the host in rank order; all-reduce of the coupling buffer on the stream -- no host synchronisation, no callback.
// Every host wait that may sit behind a collective is BOUNDED (a peer that left the solve used to leave this
// rank in hipStreamSynchronize for ever): after PROXSDP_HIP_COLLECTIVE_TIMEOUT_S seconds (default 300) without progress
// this rank aborts its communicator (ncclCommAbort: its own pending collective kernels stop) and fails the solve.
class RcclComm : public ShardComm {
    Rccl& rc;
    proxsdp_stats& st;
    ncclComm_t comm;
    int world = 1;
    DevBuf<double> send, recv, tmp, buf;
    PinnedBuf host;
    size_t cap = 0;
    const double timeout_s = collective_timeout_s();
    bool aborted = false;
    bool enqueued = false;                // a collective of this solve may be pending on the stream
    void abort() {                        // local: the communicator is unusable afterwards; the caller destroys it
        if (rc.ok() && rc.CommAbort) (void)rc.CommAbort(comm);
        aborted = true;
    }
    double* next_gather_buffer() override { return buf.p; }
    void sum_gathered(hipStream_t s, double* Mx_dev, const int* rows_d, int nc) override {
        enqueued = true;
        rc.check(rc.AllReduce(buf.p, buf.p, (size_t)nc, ncclFloat64, ncclSum, comm, s), "ncclAllReduce");
        st.rccl_reductions++;
        scatter(s, Mx_dev, rows_d, nc, buf.p);
    }

public:
    RcclComm(void* nccl_comm, proxsdp_stats& stats) : rc(Rccl::get()), st(stats), comm(static_cast<ncclComm_t>(nccl_comm)) {
        rc.require();
        int rank = 0;
        rc.check(rc.CommCount(comm, &world), "ncclCommCount");
        rc.check(rc.CommUserRank(comm, &rank), "ncclCommUserRank");
    }
    void reduce(hipStream_t s, std::vector<double>& sums, std::vector<double>& maxs) override {
        const size_t ns = sums.size(), nm = maxs.size(), n = ns + nm, W = (size_t)world;
        if (n == 0) return;
        if (cap < n) {
            cap = std::max<size_t>(n, 64);
            send.alloc(cap); recv.alloc(cap * W); host.alloc(cap * (W + 1));
        }
        double *h = host.p, *all = h + cap;
        std::copy(sums.begin(), sums.end(), h);
        std::copy(maxs.begin(), maxs.end(), h + ns);
        PX_HIP(hipMemcpyAsync(send.p, h, n * sizeof(double), hipMemcpyHostToDevice, s));
        enqueued = true;
        rc.check(rc.AllGather(send.p, recv.p, n, ncclFloat64, comm, s), "ncclAllGather");
        PX_HIP(hipMemcpyAsync(all, recv.p, n * W * sizeof(double), hipMemcpyDeviceToHost, s));
        bounded_wait(s);
        combine_in_rank_order([&](int r) { return all + (size_t)r * n; }, world, ns, nm, sums.data(), maxs.data());
        st.rccl_reductions++;
    }
    void reduce_vec_host(hipStream_t s, std::vector<double>& v) override {
        if (tmp.n < v.size()) tmp.alloc(v.size());
        tmp.upload(v.data(), v.size(), s);
        enqueued = true;
        rc.check(rc.AllReduce(tmp.p, tmp.p, v.size(), ncclFloat64, ncclSum, comm, s), "ncclAllReduce");
        tmp.download(v.data(), v.size(), s);
        bounded_wait(s);
        st.rccl_reductions++;
    }
    void setup_coupling(size_t nc, hipStream_t) override { buf.alloc(nc); }
    bool bounded_wait(hipStream_t s) override {
        const double t0 = now_s();
        poll_ready([&]() { return hipStreamQuery(s); }, [&]() {
            if (now_s() - t0 <= timeout_s) return;
            abort();
            throw std::runtime_error("block-sharded solve: a collective did not complete within " +
                                     std::to_string((int)timeout_s) + " s (did another shard leave the solve?)");
        });
        return true;
    }
    // (an argument error raised before the first collective leaves the caller's communicator usable)
    bool abort_if_pending() override {
        if (!aborted && enqueued) abort();
        return aborted;
    }
};

// In-process group: scalar records through process memory; the coupling rows by ONE kernel per shard that reads every
// shard's gathered partials through the peers' device pointers (or pinned host memory when some pair of devices has no
// peer access).  The partials are double-buffered by the parity of the call counter: a shard overwrites a buffer only after a
// later barrier, which every peer reaches after its own sum kernel of this call has finished (it synchronises before it).
class GroupComm : public ShardComm {
    ShardGroup& g;
    const int rank;
    const bool spin;
    unsigned long long calls = 0;         // reduce_coupling calls so far: their parity picks the partial buffer
    int par = 0;
    DevBuf<double> part_d[2];             // this shard's gathered partials, double-buffered
    PinnedBuf part_h[2];                  // ... staged in pinned host memory when a pair of devices has no peer access
    DevBuf<const double*> tab_d;          // [parity][shard] -> partial buffer, filled after the first barrier
    double* next_gather_buffer() override { return part_d[par = (int)(calls++ & 1)].p; }
    // finish this shard's partials (stream synchronisation), meet the peers, then sum every shard's partials into M x
    void sum_gathered(hipStream_t s, double* Mx_dev, const int* rows_d, int nc) override {
        if (g.stage_host) part_d[par].download(part_h[par].p, nc, s);
        wait_for_stream(s, spin);
        g.barrier();
        const int S = g.size();
        if (tab_d.p == nullptr) {                            // (every shard published its buffers before its first barrier)
            std::vector<const double*> tab;
            for (int q = 0; q < 2; ++q) tab.insert(tab.end(), g.coup_part[q].begin(), g.coup_part[q].end());
            tab_d.alloc(tab.size());
            PX_HIP(hipMemcpy(tab_d.p, tab.data(), tab.size() * sizeof(const double*), hipMemcpyHostToDevice));
        }
        launch_coupling_sum(s, tab_d.p + (size_t)par * S, S, rows_d, nc, Mx_dev);
    }

public:
    GroupComm(ShardGroup& group, int group_rank, bool host_wait_spin) : g(group), rank(group_rank), spin(host_wait_spin) {}
    void reduce(hipStream_t, std::vector<double>& sums, std::vector<double>& maxs) override { g.reduce(rank, sums, maxs); }
    void reduce_vec_host(hipStream_t, std::vector<double>& v) override { g.reduce_vec(rank, v); }
    // this shard's two partial buffers, published to the peers; peer access to every other device of the group, enabled once
    void setup_coupling(size_t nc, hipStream_t s) override {
        for (int q = 0; q < 2; ++q) {
            part_d[q].alloc(nc); part_d[q].zero(s);
            if (g.stage_host) part_h[q].alloc(nc, hipHostMallocPortable | hipHostMallocMapped);
            g.coup_part[q][rank] = g.stage_host ? part_h[q].p : part_d[q].p;
        }
        const auto first = g.device.begin();
        for (auto d = first; d != g.device.end() && !g.stage_host; ++d) {
            if (*d == g.device[rank] || std::find(first, d, *d) != d) continue;     // (this device, or one already enabled)
            const hipError_t e = hipDeviceEnablePeerAccess(*d, 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            else PX_HIP(e);
        }
        PX_HIP(hipStreamSynchronize(s));
    }
};

}  // namespace proxsdp
