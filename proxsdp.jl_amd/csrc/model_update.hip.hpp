// Data of a model handle replaced in place (proxsdp_hip_model_update; model.hip.hpp).  No line of the reference stands behind
// this file: ProxSDP rebuilds AffineSets, ConicSets and every workspace per optimize! (/root/reference/src/MOI_wrapper.jl:220-342),
// so a changed coefficient costs a whole set-up there.  Here the caller's new c, b, h and nzval arrays go through the maps
// prepare() recorded (variable order, off-diagonal flags, the position of every stored entry in the reordered CSC and in the
// CSR) straight into the device arrays the loop and the exit path read.
//
// Exactness.  Compiled with contraction off, like exit_device.hip.hpp.  Every stored value is ONE product of the caller's
// number with the column factor -- v * sc with sc = sqrt(2)/2 on off-diagonal PSD columns and 1.0 elsewhere, as
// finish_matrix forms it; v * cte on off-diagonal entries of c and v itself elsewhere, as prepare() does -- so the arrays
// equal a fresh prepare()'s bit for bit.  The sums of squares of the device route (k_model_norm2) run in an order fixed by
// the kernel's constants alone.
//
// Shapes (gfx950).  All four kernels are one pass of 8-40 bytes per entry, once per update: the reads of the caller's array
// and of the maps are contiguous per wavefront; k_model_values' four stores are scattered by the permutations and
// k_model_c's load follows `ord` -- nothing to tile, the passes are a few microseconds beside a solve.
#pragma once
#include "solver.hip.hpp"

namespace proxsdp {
namespace dev {

constexpr int MODEL_NORM_CHUNK = 4096;      // entries behind one partial of k_model_norm2 (TPB threads x 16 entries)

#pragma clang fp contract(off)
// entry q of the caller's values (`cnt` of them; the maps start at this array's first entry): unscaled into the exit path's
// CSC / CSR values, times its column's factor into the loop's
__global__ void __launch_bounds__(TPB)
k_model_values(const double* __restrict__ src, long long cnt, const int* __restrict__ csc_pos, const int* __restrict__ csr_pos,
               const int* __restrict__ csr_col, const unsigned char* __restrict__ offdiag, double cte,
               double* __restrict__ cval, double* __restrict__ rval, double* __restrict__ csc_val, double* __restrict__ csr_val) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < cnt; q += stride) {
        const double v = src[q];
        const int cp = csc_pos[q], rp = csr_pos[q];
        const double sc = offdiag[csr_col[rp]] ? cte : 1.0;
        const double s = v * sc;
        cval[cp] = v; rval[rp] = v;
        csc_val[cp] = s; csr_val[rp] = s;
    }
}

// position k of the solver's order takes the caller's c[ord[k]]: unscaled into the exit path's c, scaled into the loop's c
// and -- where k is in the support (sinv[k] >= 0; sinv may be null: no support path) -- into the compact cS.  *changed counts
// the positions with an empty column whose "is zero" differs from the loop's c so far: the support set is
// {column non-empty or c != 0}, so these are the positions that enter or leave it.
__global__ void __launch_bounds__(TPB)
k_model_c(const double* __restrict__ src, const long long* __restrict__ ord, const unsigned char* __restrict__ offdiag, double cte,
          const int* __restrict__ colptr, const int* __restrict__ sinv, double* __restrict__ c, double* __restrict__ c_orig,
          double* __restrict__ cS, int* __restrict__ changed, long long n) {
    const long long stride = (long long)gridDim.x * TPB;
    int moved = 0;
    for (long long k = (long long)blockIdx.x * TPB + threadIdx.x; k < n; k += stride) {
        const double v = src[ord[k]];
        const double s = offdiag[k] ? v * cte : v;
        if (colptr[k + 1] == colptr[k] && (c[k] != 0.0) != (s != 0.0)) ++moved;
        c_orig[k] = v;
        c[k] = s;
        if (sinv != nullptr) { const int at = sinv[k]; if (at >= 0) cS[at] = s; }
    }
    if (moved) atomicAdd(changed, moved);
}

// [b; h] of the loop and of the exit path (the two are equal: an equilibrated model takes no update); b or h may be null
__global__ void __launch_bounds__(TPB)
k_model_bh(const double* __restrict__ b, long long p, const double* __restrict__ h, long long m,
           double* __restrict__ bh, double* __restrict__ bh_exit) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < p + m; i += stride) {
        const double* src = i < p ? b : h;
        if (src == nullptr) continue;
        const double v = i < p ? b[i] : h[i - p];
        bh[i] = v; bh_exit[i] = v;
    }
}

// part[j] = sum of v[i]^2 over chunk j = [j MODEL_NORM_CHUNK, (j + 1) MODEL_NORM_CHUNK): thread t adds its entries
// t, t + TPB, ... in that order, the TPB sums meet in a halving tree.  The chunk, not the grid, decides who adds what: the
// workgroups walk the chunks, so any launch width gives the same partials.
__global__ void __launch_bounds__(TPB)
k_model_norm2(const double* __restrict__ v, long long n, double* __restrict__ part) {
    __shared__ double sh[TPB];
    const long long nchunk = (n + MODEL_NORM_CHUNK - 1) / MODEL_NORM_CHUNK;
    for (long long j = blockIdx.x; j < nchunk; j += gridDim.x) {
        const long long lo = j * MODEL_NORM_CHUNK;
        const long long hi = lo + MODEL_NORM_CHUNK < n ? lo + MODEL_NORM_CHUNK : n;
        double acc = 0.0;
        for (long long i = lo + threadIdx.x; i < hi; i += TPB) acc += v[i] * v[i];
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int s = TPB / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[j] = sh[0];
        __syncthreads();
    }
}
// out[0] = part[0] + part[1] + ..., added in chunk order by one thread (the host takes the square root, as norm2 does)
__global__ void k_model_norm2_fin(const double* __restrict__ part, long long nchunk, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (long long j = 0; j < nchunk; ++j) s += part[j];
    out[0] = s;
}
#pragma clang fp contract(fast)

}  // namespace dev

// ||v||_2 of n doubles on the device, in k_model_norm2's fixed order; `grid` workgroups (<= 0: the default width).  part
// needs a slot per chunk.  The result is on the host when the call returns.
inline double model_norm2(hipStream_t stream, const double* v, long long n, DevBuf<double>& part, DevBuf<double>& out, int grid = 0) {
    if (n <= 0) return 0.0;
    const long long nchunk = (n + dev::MODEL_NORM_CHUNK - 1) / dev::MODEL_NORM_CHUNK;
    if (part.n < (size_t)nchunk) part.alloc((size_t)nchunk);
    if (out.n < 1) out.alloc(1);
    const int g = grid > 0 ? grid : (int)std::min<long long>(nchunk, 1024);
    hipLaunchKernelGGL(dev::k_model_norm2, dim3(g), dim3(dev::TPB), 0, stream, v, n, part.p);
    hipLaunchKernelGGL(dev::k_model_norm2_fin, dim3(1), dim3(dev::WAVE), 0, stream, (const double*)part.p, nchunk, out.p);
    PX_HIP(hipGetLastError());
    double h = 0.0;
    out.download(&h, 1, stream);
    PX_HIP(hipStreamSynchronize(stream));
    return std::sqrt(h);
}

}  // namespace proxsdp
