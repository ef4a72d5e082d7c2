// Wide Lanczos kernels: Krylov dimensions 256..511 (options.lanczos_wide_krylov = 1).
//
// The step kernels of kernels.hip.hpp map thread j <-> basis column j and keep up to 64 basis columns per wave in
// registers: at most 255 columns.  These kernels hold nothing in registers across columns; each step of the
// recurrence with full re-orthogonalisation (two classical Gram-Schmidt passes against the whole basis, as
// KrylovKit's orthogonaliser) is a chain of launches on the block's stream:
//   k_symv_packed            w   = A v_k                       (mat-vec partial slots, the narrow path's kernel)
//   k_lzw_dots               w   = sum of the slots / sqrt2;   per-workgroup records of h1 = V_k' w
//   k_lzw_reduce             h1  = sum of the records          (one thread per column, fixed order)
//   k_lzw_update             w'  = w - V_k h1;                 records of h2 = V_k' w' and |w'|^2
//   k_lzw_reduce             h2, |w'|^2
//   k_lzw_close              alpha_k = h1[k] + h2[k], beta_k = sqrt(|w'|^2 - |h2|^2), v_{k+1} = (w' - V_k h2)/beta_k,
//                            or stop when beta_k <= tol
// Every sum has a fixed order: two runs give identical bits.  The records use a stride of KW = 512 columns; the
// alphas / betas / control record of a wide workspace has the same stride (LZW_MAXK).
// Grid of the row kernels = nt workgroups of 64 rows (the mat-vec's tiles), 4 waves that split the basis columns
// j = wv + 4c and meet in LDS; rows >= n carry zeros.
#pragma once
#include "kernels.hip.hpp"

namespace proxsdp {
namespace dev {

constexpr int KW = 512;                 // partial-dot record stride of the wide kernels (>= krylovdim + 1)
constexpr int LZW_MAXK = 512;           // alphas / betas stride of a wide record; krylovdim + 1 <= LZW_MAXK
constexpr int LZW_NRM = KW;             // slot of the reduced |w'|^2 in a wide sum buffer (KW + 1 doubles)
// a partial-dot buffer of the wide kernels: pld records of KW columns, then the pld |w'|^2 records (pld = producers rounded
// up to 64 >= nt; it exceeds KW for sides beyond 32768)
inline size_t lzw_hpart_doubles(int pld) { return (size_t)pld * KW + (size_t)pld; }

// records of V[:, 0..k]' w for the 64 rows of this workgroup: hpart[g * KW + j]; 16 columns of a wave are reduced
// together over the lanes (fold16_all), lane j < 16 holds column wv + 4 (16 ch + j)
__device__ __forceinline__ void lzw_dots(const double* __restrict__ V, int ldv, int k, int i, double w, int lane, int wv,
                                         double* __restrict__ rec) {
    const int nch = (k + 1 + 63) / 64;
    for (int ch = 0; ch < nch; ++ch) {
        double t[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int j = wv + 4 * (16 * ch + c);
            t[c] = (j <= k) ? V[(long long)j * ldv + i] * w : 0.0;
        }
        const double hs = fold16_all(t, lane);
        const int jc = wv + 4 * (16 * ch + lane);
        if (lane < 16 && jc <= k) rec[jc] = hs;
    }
}

// this wave's share of (V[:, 0..k] h)_i over its columns j = wv + 4c (h in LDS, zero-padded to a multiple of 4 * 16)
__device__ __forceinline__ double lzw_rowdot(const double* __restrict__ V, int ldv, int k, int i, int wv,
                                             const double* __restrict__ s_h) {
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
    const int ncol = (k + 1 + 3) / 4;                // columns of this wave (padding columns have h = 0)
    int c = 0;
    for (; c + 4 <= ncol; c += 4) {
        const int j = wv + 4 * c;
        const double v0 = V[(long long)min(j, k) * ldv + i], v1 = V[(long long)min(j + 4, k) * ldv + i];
        const double v2 = V[(long long)min(j + 8, k) * ldv + i], v3 = V[(long long)min(j + 12, k) * ldv + i];
        d0 += v0 * s_h[j]; d1 += v1 * s_h[j + 4]; d2 += v2 * s_h[j + 8]; d3 += v3 * s_h[j + 12];
    }
    for (; c < ncol; ++c) {
        const int j = wv + 4 * c;
        d0 += V[(long long)min(j, k) * ldv + i] * s_h[j];
    }
    return (d0 + d1) + (d2 + d3);
}

// w = A v_k from the mat-vec slots (k_symv_collect's order), records of h1 = V_k' w
__global__ void __launch_bounds__(TPB)
k_lzw_dots(const double* __restrict__ Ppart, int nt, int npad, const double* __restrict__ V, int ldv, int k,
           double* __restrict__ wbuf, double* __restrict__ hpart, const LanczosCtl* __restrict__ ctl) {
    if (ctl->stop) return;
    __shared__ double s_acc[NWAVE][LZ_ROWS];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = blockIdx.x * LZ_ROWS + lane;
    double a0 = 0.0;
    for (int s = wv; s < nt; s += NWAVE) a0 += Ppart[(long long)s * npad + i];
    s_acc[wv][lane] = a0;
    __syncthreads();
    const double w = ((s_acc[0][lane] + s_acc[1][lane]) + (s_acc[2][lane] + s_acc[3][lane])) * INV_SQRT2;
    if (wv == 0) wbuf[i] = w;
    lzw_dots(V, ldv, k, i, w, lane, wv, hpart + (long long)blockIdx.x * KW);
}

// hsum[j] = sum over the nprod producers of hpart[g * KW + j], j <= k; with_norm: hsum[LZW_NRM] = sum of the |w'|^2
// records hpart[pld * KW + g].  One thread per column, producers in order.
__global__ void __launch_bounds__(TPB)
k_lzw_reduce(const double* __restrict__ hpart, int pld, int nprod, int k, double* __restrict__ hsum,
             const LanczosCtl* __restrict__ ctl, int with_norm) {
    if (ctl->stop) return;
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j > k + 1 || (j == k + 1 && !with_norm)) return;
    const double* __restrict__ p = (j <= k) ? hpart + j : hpart + (long long)pld * KW;   // column j, or the norm records
    const long long stride = (j <= k) ? KW : 1;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int g = 0;
    for (; g + 4 <= nprod; g += 4) {
        a0 += p[(long long)g * stride];
        a1 += p[(long long)(g + 1) * stride];
        a2 += p[(long long)(g + 2) * stride];
        a3 += p[(long long)(g + 3) * stride];
    }
    for (; g < nprod; ++g) a0 += p[(long long)g * stride];
    hsum[j <= k ? j : LZW_NRM] = (a0 + a1) + (a2 + a3);
}

// first pass applied: w' = w - V_k h1; records of h2 = V_k' w' and of |w'|^2 (at hpart[pld * KW + g])
__global__ void __launch_bounds__(TPB)
k_lzw_update(double* __restrict__ wbuf, const double* __restrict__ V, int ldv, int k, const double* __restrict__ h1,
             double* __restrict__ hpart, int pld, const LanczosCtl* __restrict__ ctl) {
    if (ctl->stop) return;
    __shared__ double s_h[KW + 64];
    __shared__ double s_acc[NWAVE][LZ_ROWS];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = blockIdx.x * LZ_ROWS + lane;
    for (int j = threadIdx.x; j < KW + 64; j += TPB) s_h[j] = (j <= k) ? h1[j] : 0.0;
    const double w = wbuf[i];
    __syncthreads();
    s_acc[wv][lane] = lzw_rowdot(V, ldv, k, i, wv, s_h);
    __syncthreads();
    const double wp = w - ((s_acc[0][lane] + s_acc[1][lane]) + (s_acc[2][lane] + s_acc[3][lane]));
    if (wv == 0) {
        wbuf[i] = wp;
        const double r = wave_sum(wp * wp);
        if (lane == 0) hpart[(long long)pld * KW + blockIdx.x] = r;
    }
    lzw_dots(V, ldv, k, i, wp, lane, wv, hpart + (long long)blockIdx.x * KW);
}

// step closed: beta^2 = |w'|^2 - |h2|^2 (every workgroup, same order), alpha_k = h1[k] + h2[k],
// V[:, k+1] = (w' - V_k h2) / beta, or stop (kstop = k + 1) when beta <= tol
__global__ void __launch_bounds__(TPB)
k_lzw_close(const double* __restrict__ wbuf, double* __restrict__ V, int ldv, int k, const double* __restrict__ h1,
            const double* __restrict__ h2, double* __restrict__ alphas, double* __restrict__ betas,
            LanczosCtl* __restrict__ ctl, double tol) {
    if (ctl->stop) return;
    __shared__ double s_h[KW + 64];
    __shared__ double s_acc[NWAVE][LZ_ROWS];
    __shared__ double s_beta;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = blockIdx.x * LZ_ROWS + lane;
    for (int j = threadIdx.x; j < KW + 64; j += TPB) s_h[j] = (j <= k) ? h2[j] : 0.0;
    const double w = wbuf[i];
    __syncthreads();
    if (wv == 0) {
        double hh = 0.0;
        for (int j = lane; j <= k; j += WAVE) hh += s_h[j] * s_h[j];
        hh = wave_sum(hh);
        if (lane == 0) s_beta = sqrt(fmax(h2[LZW_NRM] - hh, 0.0));
    }
    s_acc[wv][lane] = lzw_rowdot(V, ldv, k, i, wv, s_h);
    __syncthreads();
    const double beta = s_beta;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        alphas[k] = h1[k] + s_h[k];
        betas[k] = beta;
        // the flag is only READ by later launches (stream order)
        if (beta <= tol) { ctl->kstop = k + 1; ctl->stop = 1; }
    }
    if (beta <= tol) return;
    if (wv == 0) {
        const double wi = w - ((s_acc[0][lane] + s_acc[1][lane]) + (s_acc[2][lane] + s_acc[3][lane]));
        V[(long long)(k + 1) * ldv + i] = wi / beta;
    }
}

// Restart / final rotation for any K: out[:, c] = V[:, 0..K) U[:, c], c < ncols (U compact K x ncols, column-major);
// out[:, copy_dst] = V[:, copy_src] when copy_src >= 0 (the workgroups of column group 0).  `out` must not alias V.
// Grid = (row tiles of 64, groups of LZW_RC columns); wave wv computes columns 16 wv .. 16 wv + 15 of its group for
// the 64 rows.  K is walked in chunks of LZW_RJ: the V chunk (64 rows) and the U chunk go through LDS, every
// product is accumulated in the same order (j ascending).
constexpr int LZW_RC = 64;             // columns per workgroup (16 per wave)
constexpr int LZW_RJ = 32;             // basis columns per LDS chunk
__global__ void __launch_bounds__(TPB)
k_lzw_rotate(const double* __restrict__ V, int ldv, int K, const double* __restrict__ U, int ncols,
             double* __restrict__ out, int ldo, int copy_src, int copy_dst) {
    __shared__ double s_v[LZW_RJ][LZ_ROWS];
    __shared__ double s_u[LZW_RC][LZW_RJ + 1];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int row0 = blockIdx.x * LZ_ROWS;
    const int i = row0 + lane;
    const int c0 = blockIdx.y * LZW_RC;
    if (blockIdx.y == 0 && copy_src >= 0 && wv == 0) out[(long long)copy_dst * ldo + i] = V[(long long)copy_src * ldv + i];
    if (c0 >= ncols) return;
    double acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.0;
    for (int j0 = 0; j0 < K; j0 += LZW_RJ) {
        // V chunk: 32 x 64 doubles, 8 per thread (row = lane, column = wv + 4 q)
#pragma unroll
        for (int q = 0; q < LZW_RJ / NWAVE; ++q) {
            const int jj = wv + NWAVE * q;
            s_v[jj][lane] = (j0 + jj < K) ? V[(long long)(j0 + jj) * ldv + i] : 0.0;
        }
        // U chunk: 64 columns x 32 rows, 8 per thread
#pragma unroll
        for (int q = 0; q < LZW_RC * LZW_RJ / TPB; ++q) {
            const int t = threadIdx.x + TPB * q;
            const int c = t / LZW_RJ, jj = t % LZW_RJ;
            s_u[c][jj] = (c0 + c < ncols && j0 + jj < K) ? U[(long long)(c0 + c) * K + j0 + jj] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int jj = 0; jj < LZW_RJ; ++jj) {
            const double v = s_v[jj][lane];
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] += v * s_u[16 * wv + c][jj];
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int col = c0 + 16 * wv + c;
        if (col < ncols) out[(long long)col * ldo + i] = acc[c];
    }
}

}  // namespace dev
}  // namespace proxsdp
