// A certified dual bound of a kept model (include/proxsdp_hip.h "a certified dual bound"): the device half.  The host half --
// checks, directed rounding, the serial Cholesky, the planner of the shift search, the trace caps, the combination -- is
// dual_bound_host.hpp; this file forms the dual matrix with its error radius, reduces the dual objective and the row sums,
// and factors A(sigma) = Z~ + sigma I, which is the hot path: fp64, right-looking, blocked with panels of CHOL_NB = 64, on
// the lower triangle of a dense column-major array (ld = s, entry (i, j) at A[j * s + i]; the strict upper triangle is
// never touched).  Per panel at k0, three plain dependent launches on the caller's stream:
//   k_chol_diag    one workgroup factors the diagonal block in LDS (column by column: the pivot test, IEEE sqrt, IEEE
//                  division, the rank-one update of the block's remaining columns split over the four waves); a pivot that
//                  is not above the floor -- non-positive or NaN -- writes its column into the flag and the kernel ends
//   k_chol_panel   L21 = A21 L11^-T: a workgroup of 64 threads owns 64 rows, one per lane; L11 sits in LDS and is read as a
//                  broadcast, the row's entries sit in LDS as [column][lane] (conflict-free); x_j = (a_j - sum_{t<j} x_t
//                  l_jt) / l_jj in ascending t
//   k_chol_update  A22 -= L21 L21' on the 64 x 64 tiles of the trailing lower triangle: the two 64 x 64 operand blocks of L21
//                  are staged in LDS as [k][row], each wave owns 16 columns of the tile and four accumulators of
//                  v_mfma_f64_16x16x4_f64 over the 16 steps of k in ascending order, then C - acc is stored where i >= j
// No workgroup waits for another, no atomic touches a double, and a launch that finds the flag set returns at once, so a
// failed try costs no fault and little time.  Every entry's sum has one order, fixed by the code: the same input gives the
// same factor and the same flag on every run.  Sides that are no multiple of 64 are handled by bounds: rows and columns past
// the side are zero in LDS and never stored; nothing is padded into the matrix.  The update always has a full panel behind it
// (a short panel is the last one), so its k dimension is exactly 64.
// The certificate's theorem (Higham, ASNA 2nd ed., Theorem 10.3) holds for any summation order and with fused multiply-adds:
// contraction stays on in the factorisation and off where the header fixes bits (k_bound_dual_cone).
#pragma once
#include "model_call.hip.hpp"
#include "dual_bound_host.hpp"

namespace proxsdp {
namespace dev {

constexpr int CHOL_NB = 64;

// the next double above a finite x >= 0 (an addition of non-negative terms rounded to nearest, then this: an upper bound)
__device__ __forceinline__ double bound_next_up(double x) {
    return x < INFINITY ? __longlong_as_double(__double_as_longlong(x) + 1ll) : x;      // (inf and NaN stay what they are)
}

// y[r] = dual_eq[r] for r < p, max(dual_in[r - p], 0) beyond
__global__ void __launch_bounds__(TPB)
k_bound_y(const double* __restrict__ yeq, const double* __restrict__ yin, long long p, long long Q, double* __restrict__ y) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long r = (long long)blockIdx.x * TPB + threadIdx.x; r < Q; r += stride) {
        if (r < p) y[r] = yeq[r];
        else { const double v = yin[r - p]; y[r] = v > 0.0 ? v : 0.0; }
    }
}

#pragma clang fp contract(off)
// dc[k] exactly as k_exit_dual_cone forms it, and beside it rad[k] = gamma(cnt_k + 2) (|c[k]| + sum |val_q| |y[row_q]|), both
// halved where offdiag[k]
__global__ void __launch_bounds__(TPB)
k_bound_dual_cone(const int* __restrict__ colptr, const int* __restrict__ row, const double* __restrict__ val,
                  const double* __restrict__ y, const double* __restrict__ c, const unsigned char* __restrict__ offdiag,
                  double* __restrict__ dc, double* __restrict__ rad, long long n) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long k = (long long)blockIdx.x * TPB + threadIdx.x; k < n; k += stride) {
        double acc = 0.0, aab = 0.0;
        const int q0 = colptr[k], q1 = colptr[k + 1];
        for (int q = q0; q < q1; ++q) {
            const double yr = y[row[q]];
            acc += val[q] * yr;
            aab += fabs(val[q]) * fabs(yr);
        }
        double v = c[k] + acc;
        const double ju = (double)(q1 - q0 + 2) * 0x1p-53;
        double r = (ju / (1.0 - ju)) * (fabs(c[k]) + aab);
        if (offdiag[k]) { v = v / 2.0; r = r / 2.0; }
        dc[k] = v;
        rad[k] = r;
    }
}

// out[i] = the sum over j of |M_ij| of the symmetric matrix behind a cone's packed entries, every addition rounded up
__global__ void __launch_bounds__(TPB)
k_bound_rowsum(const double* __restrict__ packed, int s, double* __restrict__ out) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= s) return;
    double acc = 0.0;
    const long long base = (long long)i * (i + 1) / 2;
    for (int j = 0; j <= i; ++j) acc = bound_next_up(acc + fabs(packed[base + j]));
    for (long long j = i + 1; j < s; ++j) acc = bound_next_up(acc + fabs(packed[j * (j + 1) / 2 + i]));
    out[i] = acc;
}

// out[0] = -sum bh_r y_r, out[1] = sum |bh_r y_r|: ONE workgroup, thread t takes r = t, t + TPB, ... in order, then a tree
// over the threads: one order whatever the launch
__global__ void __launch_bounds__(TPB)
k_bound_objective(const double* __restrict__ bh, const double* __restrict__ y, long long Q, double* __restrict__ out) {
    __shared__ double sh[2][TPB];
    double d = 0.0, D = 0.0;
    for (long long r = threadIdx.x; r < Q; r += TPB) { const double t = bh[r] * y[r]; d -= t; D += fabs(t); }
    sh[0][threadIdx.x] = d; sh[1][threadIdx.x] = D;
    __syncthreads();
    for (int w = TPB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { sh[0][threadIdx.x] += sh[0][threadIdx.x + w]; sh[1][threadIdx.x] += sh[1][threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = sh[0][0]; out[1] = sh[1][0]; }
}
#pragma clang fp contract(fast)

// Z[i * s + j] = the cone's packed entry of (i, j) (upper triangle column by column, as k_tri_gather maps it); zdiag[i] = Z_ii
__global__ void __launch_bounds__(TPB)
k_bound_gather(const double* __restrict__ packed, int s, double* __restrict__ Z, double* __restrict__ zdiag) {
    const long long total = (long long)s * s, stride = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += stride) {
        const long long i = e / s, j = e - i * s;
        const long long lo = i < j ? i : j, hi = i < j ? j : i;
        const double v = packed[hi * (hi + 1) / 2 + lo];
        Z[e] = v;
        if (i == j) zdiag[i] = v;
    }
}

// W = Z with fl(z_ii + sigma) on the diagonal; the flag is reset to "no failure"
__global__ void __launch_bounds__(TPB)
k_chol_load(const double* __restrict__ Z, int s, double sigma, double* __restrict__ W, int* __restrict__ flag) {
    const long long total = (long long)s * s, stride = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += stride) {
        const long long i = e / s, j = e - i * s;
        const double v = Z[e];
        W[e] = i == j ? v + sigma : v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = -1;
}

// the diagonal block at k0 (nb = min(64, s - k0) columns), factored in LDS.  sA[c][r] = entry (row r, column c), r >= c.
__global__ void __launch_bounds__(TPB)
k_chol_diag(double* __restrict__ A, int s, int k0, double floor_, int* __restrict__ flag) {
    if (*flag >= 0) return;
    __shared__ double sA[CHOL_NB][CHOL_NB];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int nb = min(CHOL_NB, s - k0);
    for (int c = w; c < CHOL_NB; c += NWAVE)
        sA[c][lane] = (c < nb && lane < nb && lane >= c) ? A[(long long)(k0 + c) * s + k0 + lane] : 0.0;
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        const double piv = sA[j][j];
        if (!(piv > floor_)) {                                       // (the same LDS word in every thread: a uniform branch)
            if (threadIdx.x == 0) *flag = k0 + j;
            break;                                                   // (the columns before j are written back below: they hold L)
        }
        const double d = sqrt(piv);
        __syncthreads();                                             // every thread has read the pivot
        if (w == 0) {
            if (lane == j) sA[j][j] = d;
            else if (lane > j && lane < nb) sA[j][lane] = sA[j][lane] / d;
        }
        __syncthreads();
        const double lr = sA[j][lane];
        for (int c = j + 1 + w; c < nb; c += NWAVE)
            if (lane >= c && lane < nb) sA[c][lane] -= lr * sA[j][c];
        __syncthreads();
    }
    for (int c = w; c < nb; c += NWAVE)
        if (lane < nb && lane >= c) A[(long long)(k0 + c) * s + k0 + lane] = sA[c][lane];
}

// rows k0 + 64 + 64 b .. of the panel at k0: x L11' = a, one row per lane
__global__ void __launch_bounds__(WAVE)
k_chol_panel(double* __restrict__ A, int s, int k0, const int* __restrict__ flag) {
    if (*flag >= 0) return;
    __shared__ double sL[CHOL_NB][CHOL_NB];                          // sL[c][r] = l_rc of the diagonal block
    __shared__ double sX[CHOL_NB][CHOL_NB];                          // sX[c][lane] = entry c of the lane's row
    const int lane = threadIdx.x;
    const int row = k0 + CHOL_NB + blockIdx.x * CHOL_NB + lane;
    for (int c = 0; c < CHOL_NB; ++c) {
        sL[c][lane] = lane >= c ? A[(long long)(k0 + c) * s + k0 + lane] : 0.0;
        sX[c][lane] = row < s ? A[(long long)(k0 + c) * s + row] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < CHOL_NB; ++j) {
        double acc = sX[j][lane];
        for (int t = 0; t < j; ++t) acc -= sX[t][lane] * sL[t][j];
        sX[j][lane] = acc / sL[j][j];
    }
    if (row < s)
        for (int c = 0; c < CHOL_NB; ++c) A[(long long)(k0 + c) * s + row] = sX[c][lane];
}

// tile (I, J), I >= J, of the trailing matrix behind the panel at k0: C[i][j] -= sum_k l_ik l_jk, k = 0 .. 63 ascending.
// MFMA operands (v_mfma_f64_16x16x4_f64): a = A[row l15][k = l4], b = B[k = l4][col l15], d[reg] = D[row l4 + 4 reg][col l15].
// Here D = C' of the tile: D's row = the tile's column j (this wave's 16), D's column = the tile's row i (lanes run along i,
// the contiguous direction of the column-major array).
__global__ void __launch_bounds__(TPB)
k_chol_update(double* __restrict__ A, int s, int k0, const int* __restrict__ flag) {
    const int I = blockIdx.x, J = blockIdx.y;
    if (J > I) return;
    if (*flag >= 0) return;
    __shared__ double sI[CHOL_NB][CHOL_NB];                          // sI[k][r] = l_{i0 + r, k0 + k}
    __shared__ double sJ[CHOL_NB][CHOL_NB];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int t0 = k0 + CHOL_NB;
    const int i0 = t0 + I * CHOL_NB, j0 = t0 + J * CHOL_NB;
    for (int k = w; k < CHOL_NB; k += NWAVE) {
        const long long col = (long long)(k0 + k) * s;
        sI[k][lane] = i0 + lane < s ? A[col + i0 + lane] : 0.0;
        sJ[k][lane] = j0 + lane < s ? A[col + j0 + lane] : 0.0;
    }
    __syncthreads();
    v4f64 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int q = 0; q < CHOL_NB / 4; ++q) {
        const double a = sJ[4 * q + l4][w * 16 + l15];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sI[4 * q + l4][b * 16 + l15], acc[b], 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int j = j0 + w * 16 + l4 + 4 * reg;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + b * 16 + l15;
            if (i < s && j < s && i >= j) {
                const long long e = (long long)j * s + i;
                A[e] = A[e] - acc[b][reg];
            }
        }
    }
}

}  // namespace dev

// One factorisation of the lower triangle of W (s x s, column-major, ld = s) in place on stream st: the launches only, no
// wait.  flag (device) must hold -1; afterwards -1 = completed, else the first failing column.
inline void launch_cholesky(hipStream_t st, double* W, int64_t s, double floor, int* flag) {
    for (int64_t k0 = 0; k0 < s; k0 += dev::CHOL_NB) {
        hipLaunchKernelGGL(dev::k_chol_diag, dim3(1), dim3(dev::TPB), 0, st, W, (int)s, (int)k0, floor, flag);
        const int64_t rest = s - k0 - dev::CHOL_NB;
        if (rest <= 0) break;
        const int nt = ceil_div(rest, dev::CHOL_NB);
        hipLaunchKernelGGL(dev::k_chol_panel, dim3(nt), dim3(dev::WAVE), 0, st, W, (int)s, (int)k0, (const int*)flag);
        hipLaunchKernelGGL(dev::k_chol_update, dim3(nt, nt), dim3(dev::TPB), 0, st, W, (int)s, (int)k0, (const int*)flag);
    }
    PX_HIP(hipGetLastError());
}

// proxsdp_hip_cholesky: A (host, symmetric) + shift I through the device kernels; R_out may be null
inline int64_t device_cholesky(hipStream_t st, const double* A, int64_t s, double shift, double* R_out) {
    double nu = 0.0;
    for (int64_t i = 0; i < s; ++i) {
        double a = 0.0;
        for (int64_t j = 0; j < s; ++j) a += std::fabs(A[i * s + j]);
        nu = std::max(nu, a);
    }
    DevBuf<double> Z((size_t)(s * s)), W((size_t)(s * s));
    DevBuf<int> flag(1);
    Z.upload(A, (size_t)(s * s), st);
    hipLaunchKernelGGL(dev::k_chol_load, dim3(grid_for(s * s)), dim3(dev::TPB), 0, st, (const double*)Z.p, (int)s, shift, W.p, flag.p);
    launch_cholesky(st, W.p, s, bound_pivot_floor(nu), flag.p);
    int f = 0;
    flag.download(&f, 1, st);
    std::vector<double> L;
    if (R_out) { L.resize((size_t)(s * s)); W.download(L.data(), (size_t)(s * s), st); }
    PX_HIP(hipStreamSynchronize(st));
    if (R_out)                                                       // column-major L read row-major is R = L'
        for (int64_t c = 0; c < s; ++c)
            for (int64_t r = 0; r < s; ++r) R_out[c * s + r] = r >= c ? L[(size_t)(c * s + r)] : 0.0;
    return f;
}

// what proxsdp_hip_model_bound reads of a handle: the host mirror of the rows and, on the device, the exit path's arrays
struct BoundModel {
    const Prep& P;
    const int* csc_ptr; const int* csc_row;         // the operator's pattern, CSC
    const double* cval;                             // the caller's unscaled values in that order
    const double* bh; const double* c;              // [b; h] and c, unscaled, solver order
    const unsigned char* offdiag;
};

// proxsdp_hip_model_bound on the model's stream.  q: checked by check_bound_struct; the model is one the call serves (every
// variable in a PSD cone, not equilibrated).  Nothing of the handle is written.
inline void device_dual_bound(hipStream_t st, const BoundModel& Md, proxsdp_dual_bound& q) {
    const double t0 = now_s();
    AllocCount counting;
    const Prep& P = Md.P;
    const int64_t nb = (int64_t)P.blocks.size();
    // ---- the trace caps, from the host mirror of the current rows
    std::vector<double> T((size_t)nb);
    if (q.trace_cap) {
        std::copy(q.trace_cap, q.trace_cap + nb, T.begin());
    } else {
        std::vector<int32_t> rowcnt((size_t)std::max<int64_t>(P.Q, 1), 0);
        for (int64_t e = 0; e < P.nnz; ++e) rowcnt[(size_t)P.rowidx[(size_t)e]]++;
        for (int64_t k = 0; k < nb; ++k) {
            const BlockInfo& B = P.blocks[(size_t)k];
            T[(size_t)k] = bound_trace_cap(B.n, [&](int64_t i) { return B.off + i * (i + 3) / 2; }, P.colptr.data(), P.rowidx.data(), 0,
                                           P.val_orig.data(), rowcnt, P.b_orig.data(), P.p, k);
        }
    }
    // ---- y = [y_eq; y_in+] on the device
    const size_t q1 = (size_t)std::max<int64_t>(P.Q, 1), n1 = (size_t)std::max<int64_t>(P.n, 1);
    DevBuf<double> y(q1), stage_eq, stage_in, dc(n1), rad(n1), obj(2);
    DevBuf<int> flag(2);
    const double* yeq = q.dual_eq;
    const double* yin = q.dual_in;
    if (q.on_device) {
        const double* src[2] = {q.dual_eq, q.dual_in};
        const int64_t len[2] = {P.p, P.m};
        const char* name[2] = {"dual_eq", "dual_in"};
        require_finite_device(st, flag, 2, src, len, name, "proxsdp_dual_bound");
    } else {
        if (P.p > 0) { stage_eq.alloc((size_t)P.p); stage_eq.upload(q.dual_eq, (size_t)P.p, st); yeq = stage_eq.p; }
        if (P.m > 0) { stage_in.alloc((size_t)P.m); stage_in.upload(q.dual_in, (size_t)P.m, st); yin = stage_in.p; }
    }
    double dD[2] = {0.0, 0.0};
    if (P.Q > 0) {
        hipLaunchKernelGGL(dev::k_bound_y, dim3(grid_for(P.Q)), dim3(dev::TPB), 0, st, yeq, yin, (long long)P.p, (long long)P.Q, y.p);
        hipLaunchKernelGGL(dev::k_bound_objective, dim3(1), dim3(dev::TPB), 0, st, Md.bh, (const double*)y.p,
                           (long long)P.Q, obj.p);
        obj.download(dD, 2, st);
    }
    // ---- 1. the dual matrix and its radius
    hipLaunchKernelGGL(dev::k_bound_dual_cone, dim3(grid_for(P.n)), dim3(dev::TPB), 0, st, Md.csc_ptr, Md.csc_row,
                       Md.cval, (const double*)y.p, Md.c, Md.offdiag, dc.p, rad.p, (long long)P.n);
    PX_HIP(hipGetLastError());
    int64_t smax = 1;
    for (const BlockInfo& B : P.blocks) smax = std::max<int64_t>(smax, B.n);
    DevBuf<double> Z, W, sums((size_t)(3 * smax));
    if (smax >= 2) { Z.alloc((size_t)(smax * smax)); W.alloc((size_t)(smax * smax)); }
    std::vector<double> hs((size_t)(3 * smax));
    double factor_seconds = 0.0;
    for (int64_t k = 0; k < nb; ++k) {
        const BlockInfo& B = P.blocks[(size_t)k];
        const int64_t s = B.n;
        const int gs = ceil_div(s, dev::TPB);
        // nu and rho from the packed entries; the diagonal for delta
        hipLaunchKernelGGL(dev::k_bound_rowsum, dim3(gs), dim3(dev::TPB), 0, st, (const double*)dc.p + B.off, (int)s, sums.p);
        hipLaunchKernelGGL(dev::k_bound_rowsum, dim3(gs), dim3(dev::TPB), 0, st, (const double*)rad.p + B.off, (int)s, sums.p + smax);
        if (s >= 2)
            hipLaunchKernelGGL(dev::k_bound_gather, dim3(grid_for(s * s)), dim3(dev::TPB), 0, st, (const double*)dc.p + B.off, (int)s,
                               Z.p, sums.p + 2 * smax);
        else
            PX_HIP(hipMemcpyAsync(sums.p + 2 * smax, dc.p + B.off, sizeof(double), hipMemcpyDeviceToDevice, st));
        PX_HIP(hipGetLastError());
        for (int a = 0; a < 3; ++a)
            PX_HIP(hipMemcpyAsync(hs.data() + a * smax, sums.p + a * smax, (size_t)s * sizeof(double), hipMemcpyDeviceToHost, st));
        PX_HIP(hipStreamSynchronize(st));
        double nu = 0.0, rho = 0.0;
        bool finite = true;
        for (int64_t i = 0; i < s; ++i) {
            finite = finite && std::isfinite(hs[(size_t)i]) && std::isfinite(hs[(size_t)(smax + i)]);
            nu = std::max(nu, hs[(size_t)i]); rho = std::max(rho, hs[(size_t)(smax + i)]);
        }
        const double* zdiag = hs.data() + 2 * smax;
        q.radius[k] = finite ? rho : INFINITY;
        double delta = 0.0;
        if (!finite) {                                               // an overflow in c + M'y: nothing can be certified
            q.shift[k] = INFINITY; q.lambda_lower[k] = -INFINITY; q.factorisations[k] = 0; q.certified[k] = 0;
        } else if (s == 1) {
            q.shift[k] = 0.0; q.factorisations[k] = 0; q.certified[k] = 1;
            q.lambda_lower[k] = bound_down(zdiag[0] - rho);
        } else {
            const double floor = bound_pivot_floor(nu);
            bound_certify_cone(s, zdiag, nu, rho, [&](double sigma) {
                const double tf = now_s();
                hipLaunchKernelGGL(dev::k_chol_load, dim3(grid_for(s * s)), dim3(dev::TPB), 0, st, (const double*)Z.p, (int)s, sigma,
                                   W.p, flag.p);
                launch_cholesky(st, W.p, s, floor, flag.p);
                int f = 0;
                flag.download(&f, 1, st);
                PX_HIP(hipStreamSynchronize(st));
                factor_seconds += now_s() - tf;
                return f < 0;
            }, q.shift[k], q.lambda_lower[k], delta, q.factorisations[k], q.certified[k]);
        }
        if (q.delta) q.delta[k] = delta;
        if (q.trace_used) q.trace_used[k] = T[(size_t)k];
    }
    PX_HIP(hipStreamSynchronize(st));
    // ---- 4. the combination
    q.dual_objective = dD[0];
    q.bound = bound_combine(dD[0], dD[1], P.Q, nb, T.data(), q.lambda_lower, q.certified);
    q.bytes_allocated = counting.bytes;
    q.factor_seconds = factor_seconds;
    q.seconds = now_s() - t0;
}

}  // namespace proxsdp
