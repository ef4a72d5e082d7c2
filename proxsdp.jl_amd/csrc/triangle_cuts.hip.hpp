// The two verbs of a cutting-plane round that the row change (model_rows.hip.hpp) leaves open: SEPARATE the violated triangle
// inequalities of a PSD cone of a kept model (proxsdp_hip_model_triangles, host restatement proxsdp_host_triangle_cuts), and
// name the inequality rows that WENT SLACK (proxsdp_hip_model_inactive_rows).  No line of the reference stands behind this
// file: ProxSDP has no separation and no row management.
//
// Rows.  For i < j < k of a cone of side s and the patterns 0 (-,-,-), 1 (-,+,+), 2 (+,-,+), 3 (+,+,-)
//     v = ((s1 X_ij + s2 X_ik) + s3 X_jk) - rhs            fp64, this association, contraction off
// a row is violated when v > min_violation.  The answer is the `count` violated rows that come first in the order
// (v descending, then (i, j, k, pattern) ascending).  lin = ((i s + j) s + k) 4 + pattern is that second key as one number
// (< 2^50 for every side a cone may have), and v > min_violation >= 0 makes the bit image of v monotone, so the order is the
// descending order of ONE 128-bit key:  K = bits(v) : (2^50 - 1 - lin) << 14.
//
// Device.  dense_cone_matrix (model_call.hip.hpp) builds the dense symmetric X from the primal vector.  k_tri_sweep
// visits every triple: a workgroup owns a 64 x 64 tile of (i, j) pairs (tiles with block row <= block column, pairs with
// i >= j masked) and up to TRI_KG chunks of 64 values of k from the tile's j-block upward; the rows X[k, I] and X[k, J] of a
// chunk are staged in LDS (X is symmetric: the tile [k][row] is read from global memory along `row`, contiguously, and read
// from LDS by a wave as 4 broadcast addresses of the i-tile and 16 consecutive doubles of the j-tile: no bank conflict, no
// padding); each lane keeps a 4 x 4 register tile of X_ij.  Masked pairs and rows past the side hold NaN, which violates
// nothing, so only the chunk that holds the tile's own j needs the j < k test.  Selection is a radix select on K in digits of
// TRI_DIGIT_BITS bits: a histogram sweep counts, for the rows whose higher digits equal the prefix fixed so far, the next
// digit in LDS-private bins flushed with integer atomics (the counts are exact whatever the launch); the host fixes the digit
// where the running count from the top crosses `count`; once the rows at or above the prefix number at most cand_cap, an emit
// sweep appends them with their keys through an atomic cursor and the host sorts them.  The append order is arbitrary, the
// set and the sort are not: the result is a pure function of the inputs.  Scratch: X, TRI_BINS counters, 2 cand_cap words.
// Only the first pass looks at every violated row; from the second on a row enters the bookkeeping when v passes the gate that
// the prefix implies (tri_gate), and while the digit lies inside the bits of v the index is not formed at all.
// The host half -- argument checks, the order, the decoding of a row, the serial restatement, the gate -- is
// triangle_cuts_host.hpp, which needs no HIP.
#pragma once
#include "model_call.hip.hpp"
#include "triangle_cuts_host.hpp"

namespace proxsdp {

constexpr int TRI_TILE = 64;                    // side of a workgroup's (i, j) tile and length of a chunk of k
constexpr int TRI_KG = 8;                       // chunks of k per workgroup
constexpr int INACT_TPB = 1024;

// the low word of K: ascending lin is descending K
__host__ __device__ inline unsigned long long tri_key_lo(unsigned long long lin) {
    return ((~lin) & (((unsigned long long)1 << TRI_LIN_BITS) - 1)) << TRI_LIN_SHIFT;
}

namespace dev {

// one row past the gate.  MODE 0: its digit is counted when the higher digits equal P, the digit lying inside the bits of v
// (shift >= 64: lin is not needed and never formed); MODE 2: the same for any digit; MODE 1: the row is appended when its
// leading digits are >= P
template <int MODE>
__device__ __forceinline__ void tri_row(double v, unsigned long long lin, int shift, tri_u128 P, unsigned* bins,
                                        unsigned long long* __restrict__ cand, unsigned* __restrict__ cursor, unsigned cap) {
    const unsigned long long vb = (unsigned long long)__double_as_longlong(v);
    if (MODE == 0) {
        const unsigned long long q = vb >> (shift - 64);
        if ((q >> TRI_DIGIT_BITS) == (unsigned long long)P) atomicAdd(&bins[(unsigned)q & (TRI_BINS - 1)], 1u);
        return;
    }
    const tri_u128 q = ((((tri_u128)vb) << 64) | (tri_u128)tri_key_lo(lin)) >> shift;
    if (MODE == 2) {
        if ((q >> TRI_DIGIT_BITS) == P) atomicAdd(&bins[(unsigned)q & (TRI_BINS - 1)], 1u);
    } else {
        if (q >= P) {
            const unsigned pos = atomicAdd(cursor, 1u);
            if (pos < cap) { cand[2 * (size_t)pos] = vb; cand[2 * (size_t)pos + 1] = lin; }
        }
    }
}

#pragma clang fp contract(off)
// the 64 values of k of one staged chunk against the lane's 4 x 4 pairs.  CHECKJ: the chunk holds the tile's own j
template <int MODE, bool CHECKJ>
__device__ __forceinline__ void tri_chunk(const double (*TI)[TRI_TILE], const double (*TJ)[TRI_TILE], const double (&xij)[4][4],
                                          int ti, int tj, int I0, int J0, int kc, int s, double gate, double rhs, int shift,
                                          tri_u128 P, unsigned* bins, unsigned long long* __restrict__ cand,
                                          unsigned* __restrict__ cursor, unsigned cap) {
    double xi[4], xj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { xi[a] = TI[0][ti + 16 * a]; xj[a] = TJ[0][tj + 16 * a]; }
#pragma unroll 1
    for (int kk = 0; kk < TRI_TILE; ++kk) {
        double ci[4], cj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { ci[a] = xi[a]; cj[a] = xj[a]; }
        const int kn = kk + 1 < TRI_TILE ? kk + 1 : kk;             // the next k's values while this one's are worked on
#pragma unroll
        for (int a = 0; a < 4; ++a) { xi[a] = TI[kn][ti + 16 * a]; xj[a] = TJ[kn][tj + 16 * a]; }
        const int k = kc + kk;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double A = xij[a][b], B = ci[a], C = cj[b];
                const double v0 = ((-A - B) - C) - rhs;
                const double v1 = ((-A + B) + C) - rhs;
                const double v2 = ((A - B) + C) - rhs;
                const double v3 = ((A + B) - C) - rhs;
                const double vm = fmax(fmax(v0, v1), fmax(v2, v3));
                const bool ok = !CHECKJ || (J0 + tj + 16 * b < k);
                if (ok && vm > gate) {
                    const unsigned long long i = (unsigned long long)(I0 + ti + 16 * a), j = (unsigned long long)(J0 + tj + 16 * b);
                    const unsigned long long lin = ((i * (unsigned long long)s + j) * (unsigned long long)s + (unsigned long long)k) * 4ull;
                    if (v0 > gate) tri_row<MODE>(v0, lin, shift, P, bins, cand, cursor, cap);
                    if (v1 > gate) tri_row<MODE>(v1, lin + 1, shift, P, bins, cand, cursor, cap);
                    if (v2 > gate) tri_row<MODE>(v2, lin + 2, shift, P, bins, cand, cursor, cap);
                    if (v3 > gate) tri_row<MODE>(v3, lin + 3, shift, P, bins, cand, cursor, cap);
                }
            }
    }
}
#pragma clang fp contract(fast)

// grid: x = tiles (bi <= bj) of the nt x nt tile grid, column by column; y = groups of TRI_KG chunks of k from chunk bj upward.
// gate: a row is looked at when v > gate -- min_violation, or the larger of it and the value just below the smallest v the prefix
// P admits (tri_gate): the rows of a later pass are few, and the sweep then runs at the rate of its arithmetic.
// MODE 0 / 2: hist[TRI_BINS] += the digit counts (shift = 128 - TRI_DIGIT_BITS (d + 1), P = the d digits fixed so far; 0 while
// the digit lies in the bits of v, 2 from there on); MODE 1: the rows with K >> shift >= P into cand (vb, lin per entry) at
// cursor, cap entries at the most.
template <int MODE>
__global__ void __launch_bounds__(TPB)
k_tri_sweep(const double* __restrict__ X, int s, int nt, double gate, double rhs, int shift, unsigned long long p_hi,
            unsigned long long p_lo, unsigned long long* __restrict__ hist, unsigned long long* __restrict__ cand,
            unsigned* __restrict__ cursor, unsigned cap) {
    __shared__ double TI[TRI_TILE][TRI_TILE], TJ[TRI_TILE][TRI_TILE];
    __shared__ unsigned bins[MODE != 1 ? TRI_BINS : 1];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int t = blockIdx.x;
    int bj = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((bj + 1) * (bj + 2) / 2 <= t) ++bj;
    while (bj * (bj + 1) / 2 > t) --bj;
    const int bi = t - bj * (bj + 1) / 2;
    const int c0 = bj + (int)blockIdx.y * TRI_KG;
    if (c0 >= nt) return;                                           // (the whole workgroup: before any barrier)
    const int c1 = c0 + TRI_KG < nt ? c0 + TRI_KG : nt;
    const int I0 = bi * TRI_TILE, J0 = bj * TRI_TILE;
    const tri_u128 P = (((tri_u128)p_hi) << 64) | (tri_u128)p_lo;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (MODE != 1)
        for (int b = tid; b < TRI_BINS; b += TPB) bins[b] = 0u;
    double xij[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = I0 + ti + 16 * a, j = J0 + tj + 16 * b;
            xij[a][b] = (i < j && j < s) ? X[(long long)i * s + j] : nan;
        }
    for (int c = c0; c < c1; ++c) {
        const int kc = c * TRI_TILE;
        __syncthreads();                                            // the previous chunk is done with the tiles (first: bins are 0)
        const int r = tid & 63;
#pragma unroll 4
        for (int q = 0; q < TRI_TILE / 4; ++q) {
            const int kk = (tid >> 6) + 4 * q, k = kc + kk;
            TI[kk][r] = (k < s && I0 + r < s) ? X[(long long)k * s + I0 + r] : nan;
            TJ[kk][r] = (k < s && J0 + r < s) ? X[(long long)k * s + J0 + r] : nan;
        }
        __syncthreads();
        if (c == bj) tri_chunk<MODE, true>(TI, TJ, xij, ti, tj, I0, J0, kc, s, gate, rhs, shift, P, bins, cand, cursor, cap);
        else tri_chunk<MODE, false>(TI, TJ, xij, ti, tj, I0, J0, kc, s, gate, rhs, shift, P, bins, cand, cursor, cap);
    }
    if (MODE != 1) {
        __syncthreads();
        for (int b = tid; b < TRI_BINS; b += TPB)
            if (bins[b]) atomicAdd(&hist[b], (unsigned long long)bins[b]);
    }
}

// rows[0 .. *count) = the r < m with |dual[r]| <= dual_tol and slack[r] < -slack_tol, ascending (a NaN fails both tests).
// ONE workgroup walks the rows in pieces of INACT_TPB: a piece's flags are ranked by ballots and a scan of the waves' counts,
// and the pieces follow each other, so the order is the rows' own, whatever the launch.
__global__ void __launch_bounds__(INACT_TPB)
k_inactive_rows(const double* __restrict__ dual, const double* __restrict__ slack, long long m, double dual_tol,
                double slack_tol, long long* __restrict__ rows, long long* __restrict__ count) {
    __shared__ int wcnt[INACT_TPB / 64];
    __shared__ long long base_sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) base_sh = 0;
    __syncthreads();
    for (long long r0 = 0; r0 < m; r0 += INACT_TPB) {
        const long long r = r0 + tid;
        const bool f = r < m && fabs(dual[r]) <= dual_tol && slack[r] < -slack_tol;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) wcnt[w] = __popcll(bal);
        __syncthreads();
        long long off = base_sh;
        for (int q = 0; q < w; ++q) off += wcnt[q];
        if (f) rows[off + __popcll(bal & (((unsigned long long)1 << lane) - 1))] = r;
        __syncthreads();
        if (tid == 0) {
            long long tot = 0;
            for (int q = 0; q < INACT_TPB / 64; ++q) tot += wcnt[q];
            base_sh += tot;
        }
        __syncthreads();
    }
    if (tid == 0) *count = base_sh;
}

}  // namespace dev

// proxsdp_hip_model_triangles on the model's stream.  ord_h / ord_d: the cone's variable list (0-based caller numbers) on the
// host and on the device; n: the model's variables; tc: checked by check_triangle_struct
inline void device_triangle_cuts(hipStream_t st, const int64_t* ord_h, const long long* ord_d, int64_t s, int base, int cone,
                                 proxsdp_triangle_cuts& tc) {
    const double t0 = now_s();
    AllocCount counting;
    const unsigned cap = (unsigned)std::max<int64_t>(tc.cand_cap > 0 ? tc.cand_cap : std::max<int64_t>(4 * tc.count, 65536), tc.count);
    const DevBuf<double> X = dense_cone_matrix(st, tc.primal, tc.on_device != 0, ord_h, ord_d, s,
                                               "proxsdp_triangle_cuts: non-finite entry of primal in cone " + std::to_string(cone));
    DevBuf<unsigned long long> hist((size_t)TRI_BINS), cand((size_t)2 * cap);
    DevBuf<unsigned> cursor(1);
    const int nt = (int)((s + TRI_TILE - 1) / TRI_TILE);
    const dim3 grid((unsigned)(nt * (nt + 1) / 2), (unsigned)((nt + TRI_KG - 1) / TRI_KG));
    StreamTimer first_pass(st);
    int passes = 0;
    // mode 0: histogram, 1: emit; P holds 128 - shift bits (hist: less the digit's)
    auto sweep = [&](int mode, int shift, tri_u128 P) {
        const unsigned long long hi = (unsigned long long)(P >> 64), lo = (unsigned long long)P;
        const int pbits = 128 - shift - (mode == 0 ? TRI_DIGIT_BITS : 0);
        const double gate = tri_gate(tc.min_violation, P, pbits);
        if (passes == 0) first_pass.start();
        if (mode == 0) {
            hist.zero(st);
            if (shift >= 64)
                hipLaunchKernelGGL(dev::k_tri_sweep<0>, grid, dim3(dev::TPB), 0, st, (const double*)X.p, (int)s, nt, gate,
                                   tc.rhs, shift, hi, lo, hist.p, cand.p, cursor.p, cap);
            else
                hipLaunchKernelGGL(dev::k_tri_sweep<2>, grid, dim3(dev::TPB), 0, st, (const double*)X.p, (int)s, nt, gate,
                                   tc.rhs, shift, hi, lo, hist.p, cand.p, cursor.p, cap);
        } else {
            cursor.zero(st);
            hipLaunchKernelGGL(dev::k_tri_sweep<1>, grid, dim3(dev::TPB), 0, st, (const double*)X.p, (int)s, nt, gate,
                               tc.rhs, shift, hi, lo, hist.p, cand.p, cursor.p, cap);
        }
        PX_HIP(hipGetLastError());
        if (passes == 0) first_pass.stop();
        ++passes;
    };
    std::vector<unsigned long long> h((size_t)TRI_BINS);
    tri_u128 P = 0;
    unsigned long long above = 0, expect = 0, violated = 0;
    const unsigned long long count = (unsigned long long)tc.count;
    bool emitted = false;
    for (int d = 0; d < TRI_DIGITS && !emitted; ++d) {
        sweep(0, 128 - TRI_DIGIT_BITS * (d + 1), P);
        hist.download(h.data(), h.size(), st);
        PX_HIP(hipStreamSynchronize(st));
        if (d == 0) {
            for (unsigned long long c : h) violated += c;
            if (violated == 0) break;
            if (violated <= cap) { sweep(1, 127, 0); expect = violated; emitted = true; break; }     // (v > 0: bit 127 of K is 0)
        }
        unsigned long long run = 0;
        int b = TRI_BINS - 1;
        for (; b > 0; --b) {
            if (above + run + h[b] >= count) break;
            run += h[b];
        }
        above += run;
        P = (P << TRI_DIGIT_BITS) | (tri_u128)(unsigned)b;
        if (above + h[b] <= cap) { sweep(1, 128 - TRI_DIGIT_BITS * (d + 1), P); expect = above + h[b]; emitted = true; }
    }
    std::vector<TriCand> rows;
    if (emitted) {
        unsigned got = 0;
        cursor.download(&got, 1, st);
        PX_HIP(hipStreamSynchronize(st));
        if ((unsigned long long)got != expect) throw std::logic_error("proxsdp_triangle_cuts: the emit sweep and the histograms disagree");
        rows.resize(got);
        static_assert(sizeof(TriCand) == 2 * sizeof(unsigned long long), "a candidate is two words");
        if (got) PX_HIP(hipMemcpyAsync(rows.data(), cand.p, (size_t)got * sizeof(TriCand), hipMemcpyDeviceToHost, st));
        PX_HIP(hipStreamSynchronize(st));
    } else if (violated != 0) {
        throw std::logic_error("proxsdp_triangle_cuts: the radix select did not end");
    }
    tri_write_rows(rows, s, tc, [&](int64_t i, int64_t j) { return ord_h[j * (j + 1) / 2 + i] + base; });
    tc.violated = (int64_t)violated; tc.scanned = tri_scanned(s); tc.passes = passes;
    tc.sweep_seconds = first_pass.seconds();
    tc.bytes_allocated = counting.bytes;
    tc.seconds = now_s() - t0;
}

// ---- rows that went slack
inline void inactive_rows(hipStream_t st, int64_t m, proxsdp_inactive_rows& q) {
    q.n_rows = 0;
    if (m == 0) return;
    if (!q.on_device) { inactive_rows_host(m, q); return; }
    DevBuf<long long> rows((size_t)m), cnt(1);
    hipLaunchKernelGGL(dev::k_inactive_rows, dim3(1), dim3(INACT_TPB), 0, st, q.dual_in, q.slack_in, (long long)m, q.dual_tol,
                       q.slack_tol, rows.p, cnt.p);
    PX_HIP(hipGetLastError());
    long long got = 0;
    cnt.download(&got, 1, st);
    PX_HIP(hipStreamSynchronize(st));
    static_assert(sizeof(long long) == sizeof(int64_t), "the row numbers are downloaded as they are");
    rows.download(reinterpret_cast<long long*>(q.rows), (size_t)got, st);
    PX_HIP(hipStreamSynchronize(st));
    q.n_rows = got;
}

}  // namespace proxsdp
