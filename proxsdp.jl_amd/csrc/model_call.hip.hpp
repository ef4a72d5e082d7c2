// What a call on a model handle needs round its kernels (model.hip.hpp; DESIGN.md "The call path of a handle tool"): the
// count of the call's own device allocations, an event timer on the model's stream, the finite check of data the caller holds
// on the device (require_finite_device, exit_device.hip.hpp) and the dense matrix of a PSD cone.  A tool header includes this
// file itself.  No line of the reference stands behind it.
#pragma once
#include "exit_device.hip.hpp"

namespace proxsdp {

// the device bytes this thread allocates while one lives: a call's bytes_allocated
struct AllocCount {
    long long bytes = 0;
    long long* prev;
    AllocCount() : prev(DevAccount::allocated) { DevAccount::allocated = &bytes; }
    ~AllocCount() { DevAccount::allocated = prev; }
    AllocCount(const AllocCount&) = delete;
    AllocCount& operator=(const AllocCount&) = delete;
};

// Seconds the stream spent between start() and stop(), summed over the intervals.  An interval is read once its events have
// completed: by the next start() or by seconds(), so the stream is synchronised before either.
struct StreamTimer {
    hipStream_t st;
    Event ev0, ev1;
    double ms = 0.0;
    bool open = false;                          // an interval recorded and not yet read
    explicit StreamTimer(hipStream_t s) : st(s) { ev0.create(); ev1.create(); }
    void start() { read(); PX_HIP(hipEventRecord(ev0, st)); }
    void stop() { PX_HIP(hipEventRecord(ev1, st)); open = true; }
    double seconds() { read(); return ms * 1e-3; }
    void read() {
        if (!open) return;
        float t = 0.f;
        PX_HIP(hipEventElapsedTime(&t, ev0, ev1));
        ms += (double)t;
        open = false;
    }
};

namespace dev {

// X[i, j] = X[j, i] = primal[ord[tri_index(min, max)]]: ord = the cone's variable list (upper triangle, column by column)
__global__ void __launch_bounds__(TPB)
k_tri_gather(const double* __restrict__ primal, const long long* __restrict__ ord, int s, double* __restrict__ X) {
    const long long total = (long long)s * s, stride = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += stride) {
        const long long i = e / s, j = e - i * s;
        const long long lo = i < j ? i : j, hi = i < j ? j : i;
        X[e] = primal[ord[hi * (hi + 1) / 2 + lo]];
    }
}

}  // namespace dev

// The dense symmetric X (s x s) of a cone from the primal vector, finite or refused with `message`.  ord_h / ord_d: the cone's
// variable list (0-based caller numbers) on the host and on the device.  Device vector: gathered, then checked; host vector:
// checked before anything is allocated, expanded, uploaded.
inline DevBuf<double> dense_cone_matrix(hipStream_t st, const double* primal, bool on_device, const int64_t* ord_h,
                                        const long long* ord_d, int64_t s, const std::string& message) {
    DevBuf<double> X;
    if (on_device) {
        X.alloc((size_t)(s * s));
        DevBuf<int> flag(1);
        hipLaunchKernelGGL(dev::k_tri_gather, dim3(grid_for(s * s)), dim3(dev::TPB), 0, st, primal, ord_d, (int)s, X.p);
        require_finite_device(st, flag, X.p, s * s, message);
    } else {
        for (int64_t e = 0; e < s * (s + 1) / 2; ++e)
            if (!std::isfinite(primal[ord_h[e]])) throw std::invalid_argument(message);
        X.alloc((size_t)(s * s));
        std::vector<double> Xh((size_t)(s * s));
        for (int64_t j = 0; j < s; ++j)
            for (int64_t i = 0; i <= j; ++i) Xh[i * s + j] = Xh[j * s + i] = primal[ord_h[j * (j + 1) / 2 + i]];
        X.upload(Xh.data(), Xh.size(), st);
        PX_HIP(hipStreamSynchronize(st));
    }
    return X;
}

}  // namespace proxsdp
