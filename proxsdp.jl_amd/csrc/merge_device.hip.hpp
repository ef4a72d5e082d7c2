// Rank-one merge of the split K x K eigensolve on the DEVICE (options.device_eig_merge): the O(k^2) part of
// host_eig_merge.hpp -- secular roots, Gu-Eisenstat weights, secular eigenvectors, the product with Qf -- as short
// dependent launches on the solver's stream, so that the Ritz-vector coefficients never visit the host.
//
// The host keeps what is serial, cheap and delicate: the two QL decompositions (first part under the cycle, tail after
// it) and Rank1Merge::plan() -- the merged pole list, z, the deflation scan.  plan() runs WITHOUT Qf here and hands over
// the column map and the rotation list; one packed upload carries them with Q2, the poles, dn, zn, rho and betaK.
// Five launches (four when nothing rotates):
//
//   k_mg_roots     one wave per non-deflated root: Rank1Merge::solve_root statement for statement; lane l holds poles l,
//                  l+64, l+128, l+192 and computes their terms, lanes 0..3 add psi, dpsi, phi, dphi up in pole order;
//                  lam, iteration count, row of delta.  The same launch assembles Qf (K x K) from Q1 | Q2 by the column
//                  map, one workgroup per column: the two are independent and a launch of their own would only add latency
//   k_mg_rotate    the deflation rotations on Qf in list order (thread = row); launched only when the plan has any
//   k_mg_weights   one wave per pole: the Loewner product with the host's pairing of ratios, multiplied up in its order -> zhat
//   k_mg_vectors   one wave per eigenvalue of T (roots, then deflated poles): s = zhat / delta_row normalised, the last
//                  row of the eigenvectors of T, and the position in DESCENDING order by counting (ties as the host's
//                  stable_sort); writes the record  f = betaK x last row | D | status  in the layout k_lz_orth reads its
//                  arrow part in, so that a restart needs no upload
//   (record -> pinned host memory)
//   k_mg_eigvecs   Uall[:, c] = Qf[:, nd] S[:, root] (pole order; FMA or multiply-add per row as the host's panels) or the
//                  Qf column of a deflated pole, all K columns in descending order: what the rotation kernels take as U.
//                  It runs behind the record's copy, while the host reads D and f.
//
// THE SAME BITS AS THE HOST MERGE.  Every sum and product runs in Rank1Merge's order (the independent terms in parallel,
// the additions serially on one lane), contraction is off in every kernel, and fp64 division and square root are
// correctly rounded on both sides: lam, D, f and U equal the host's as bit patterns (tests/test_device_merge.py), so a
// solve does not depend on who merged -- a fallback in the middle of one included.  No floating-point atomics, no
// waiting on another workgroup, every loop bounded.
#pragma once

namespace proxsdp {
namespace dev {

constexpr int MG_KMAX = 255;                  // largest K served (the step kernels' largest Krylov dimension)
constexpr int MG_LD = 256;                    // stride of the per-pole arrays of the packed upload
// packed upload, in doubles: [ints: K k1 k2 k ndf nrot host-fma . | colsrc | nd | df | rot pj | rot j]
//                            [rho betaK | d | dn | zn | rot c | rot s] [Q2 (k2 x k2)]
constexpr int MG_I_COLSRC = 8, MG_I_ND = MG_I_COLSRC + MG_LD, MG_I_DF = MG_I_ND + MG_LD, MG_I_RPJ = MG_I_DF + MG_LD,
              MG_I_RJ = MG_I_RPJ + MG_LD, MG_NINT = MG_I_RJ + MG_LD;
constexpr int MG_SC = MG_NINT / 2, MG_D = MG_SC + 2, MG_DN = MG_D + MG_LD, MG_ZN = MG_DN + MG_LD, MG_RC = MG_ZN + MG_LD,
              MG_RS = MG_RC + MG_LD, MG_Q2 = MG_RS + MG_LD, MG_PACK = MG_Q2 + (MG_KMAX - 1) * (MG_KMAX - 1);
static_assert(MG_NINT % 2 == 0, "the int part of the pack ends on a double");
// record: f [MAXK] | D [MAXK] | status (k_lz_orth reads its arrow part as f at 0, D at MAXK)
constexpr int MG_REC = 2 * MAXK + 8;
constexpr double MG_TINY = 2.2250738585072014e-308;        // std::numeric_limits<double>::min()

// The host merge sums serially, and the device merge returns the host's bits: the terms of a sum are independent (one
// division each) and go to the lanes; the ADDITIONS then run in the host's order on one lane, from a staging row in LDS.
// A chain of k dependent adds is ~8 cycles a link -- what the divisions in front of it cost -- where a tree would give
// other bits than the merge every golden trace of the suite was written with.
__device__ __forceinline__ void mg_stage_sync() {            // the wave's LDS writes are visible to its own lanes
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}
template <int L>
__device__ __forceinline__ double mg_from_lane(double v) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), L);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), L);
    return __hiloint2double(hi, lo);
}
// st[lo] + st[lo + 1] + ... in that order, from 0.0: a serial loop's additions
__device__ __forceinline__ double mg_serial_sum(const double* st, int lo, int hi) {
#pragma clang fp contract(off)
    double a = 0.0;
#pragma unroll 8
    for (int j = lo; j < hi; ++j) a += st[j];
    return a;
}
__device__ __forceinline__ int mg_wave_count(int v) { return (int)wave_sum((double)v); }   // (small counts: exact)

// column p of Qf from its source column of Q1 (rows [0, k1)) or Q2 (rows [k1, K)): the second part of k_mg_roots' grid
__device__ __forceinline__ void mg_assemble_column(const double* __restrict__ pack, const double* __restrict__ Q1,
                                                   double* __restrict__ Qf, int p) {
    const int* hi = reinterpret_cast<const int*>(pack);
    const int K = hi[0], k1 = hi[1], k2 = hi[2];
    const int cs = hi[MG_I_COLSRC + p];
    const double* src = cs >= 0 ? Q1 + (size_t)cs * k1 : pack + MG_Q2 + (size_t)(-(cs + 1)) * k2;
    for (int r = threadIdx.x; r < K; r += blockDim.x) {
        double v = 0.0;
        if (cs >= 0) { if (r < k1) v = src[r]; }
        else if (r >= k1) v = src[r - k1];
        Qf[(size_t)p * K + r] = v;
    }
}

// the deflation rotations in list order, thread = row (launched only when the plan has any: typically 0-3)
__global__ __launch_bounds__(64) void k_mg_rotate(const double* __restrict__ pack, double* __restrict__ Qf) {
#pragma clang fp contract(off)
    const int* hi = reinterpret_cast<const int*>(pack);
    const int K = hi[0], nrot = hi[5];
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= K) return;
    // (a thread reads back only what it wrote itself: row r of two columns)
    for (int q = 0; q < nrot; ++q) {
        const int pj = hi[MG_I_RPJ + q], j = hi[MG_I_RJ + q];
        const double c = pack[MG_RC + q], s = pack[MG_RS + q];
        const double xr = Qf[(size_t)pj * K + r], yr = Qf[(size_t)j * K + r];
        Qf[(size_t)pj * K + r] = c * xr + s * yr;
        Qf[(size_t)j * K + r] = c * yr - s * xr;
    }
}

// the secular function on this lane's poles at lambda = dn[org] + tau (Rank1Merge::eval): psi = poles <= isplit, phi = the rest.
// sp / sq: this wave's staging rows.  Lanes 0..3 fold psi, dpsi, phi, dphi in pole order.
__device__ __forceinline__ void mg_eval(const double (&dnl)[4], const double (&znl)[4], int lane, int k, double dorg, double tau,
                                        int isplit, double rho, double* sp, double* sq, double& psi, double& dpsi, double& phi,
                                        double& dphi) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
        if (j < k) {
            const double dl = (dnl[q] - dorg) - tau;
            const double t = znl[q] / dl;
            sp[j] = znl[q] * t; sq[j] = t * t;
        }
    }
    mg_stage_sync();
    double acc = 0.0;
    if (lane < 4) acc = mg_serial_sum((lane & 1) ? sq : sp, lane < 2 ? 0 : isplit + 1, lane < 2 ? isplit + 1 : k);
    mg_stage_sync();
    psi = rho * mg_from_lane<0>(acc); dpsi = rho * mg_from_lane<1>(acc);
    phi = rho * mg_from_lane<2>(acc); dphi = rho * mg_from_lane<3>(acc);
}

// grid = ceil(k / 4) workgroups of four roots, then K workgroups that assemble one column of Qf each: the two are
// independent, so they share a launch and the columns fill the CUs the roots leave idle
__global__ __launch_bounds__(256) void k_mg_roots(const double* __restrict__ pack, const double* __restrict__ Q1,
                                                  double* __restrict__ Qf, double* __restrict__ lam,
                                                  double* __restrict__ delta, int* __restrict__ iters) {
#pragma clang fp contract(off)
    const int* hi = reinterpret_cast<const int*>(pack);
    const int k = hi[3];
    const int nrb = (k + 3) >> 2;
    if ((int)blockIdx.x >= nrb) {
        if ((int)blockIdx.x - nrb < hi[0]) mg_assemble_column(pack, Q1, Qf, (int)blockIdx.x - nrb);
        return;
    }
    __shared__ double s_st[4][2][MG_LD];
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= k) return;                                      // (whole waves leave: no workgroup barrier below)
    double* sp = s_st[threadIdx.x >> 6][0];
    double* sq = s_st[threadIdx.x >> 6][1];
    const double* dn = pack + MG_DN;
    const double* zn = pack + MG_ZN;
    const double rho = pack[MG_SC];
    const double eps = 2.220446049250313e-16;
    double dnl[4], znl[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
        dnl[q] = j < k ? dn[j] : 0.0;
        znl[q] = j < k ? zn[j] : 0.0;
    }
    int org = 0, it = 0;
    double tau;
    if (k == 1) {
        tau = rho * zn[0] * zn[0];
    } else {
        const bool last = (i == k - 1);
        const int ia = last ? k - 2 : i, ib = ia + 1;
        const int isplit = ia;
        double lo, hi_, psi, dpsi, phi, dphi;
        if (!last) {
            const double gap = dn[i + 1] - dn[i];
            mg_eval(dnl, znl, lane, k, dn[i], 0.5 * gap, isplit, rho, sp, sq, psi, dpsi, phi, dphi);
            const double fmid = 1.0 + psi + phi;
            if (fmid >= 0.0) { org = i; lo = 0.0; hi_ = 0.5 * gap; }
            else { org = i + 1; lo = -0.5 * gap; hi_ = 0.0; }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (lane + 64 * q < k) sp[lane + 64 * q] = znl[q] * znl[q];
            mg_stage_sync();
            double zz = lane == 0 ? mg_serial_sum(sp, 0, k) : 0.0;
            mg_stage_sync();
            zz = mg_from_lane<0>(zz);
            org = k - 1; lo = 0.0; hi_ = rho * zz;
        }
        const double dorg = dn[org];
        const double dia = dn[ia] - dorg, dib = dn[ib] - dorg;
        tau = 0.5 * (lo + hi_);
        double f = 0.0;
        for (; it < 80; ++it) {
            if (!(tau > lo && tau < hi_)) tau = 0.5 * (lo + hi_);
            if (tau == lo || tau == hi_) break;
            mg_eval(dnl, znl, lane, k, dorg, tau, isplit, rho, sp, sq, psi, dpsi, phi, dphi);
            f = 1.0 + psi + phi;
            const double erretm = 8.0 * (fabs(psi) + fabs(phi)) + 2.0 + fabs(tau) * (dpsi + dphi);
            if (fabs(f) <= eps * erretm) break;
            if (f < 0.0) lo = tau; else hi_ = tau;
            if (hi_ - lo <= 2.0 * eps * fmax(fabs(lo), fabs(hi_))) { tau = 0.5 * (lo + hi_); break; }
            const double Da = dia - tau, Db = dib - tau;
            const double s = dpsi * Da * Da, Sb = dphi * Db * Db;
            const double c = f - dpsi * Da - dphi * Db;
            const double bq = c * (Da + Db) + s + Sb;
            const double w = Da * Db * f;
            double eta;
            if (c == 0.0) {
                eta = (bq != 0.0) ? w / bq : 0.0;
            } else {
                double disc = bq * bq - 4.0 * c * w;
                if (disc < 0.0) disc = 0.0;
                const double sq = sqrt(disc);
                const double qq = (bq >= 0.0) ? 0.5 * (bq + sq) : 0.5 * (bq - sq);
                const double e1 = (qq != 0.0) ? w / qq : 0.0;
                const double e2 = qq / c;
                const double t1 = tau + e1, t2 = tau + e2;
                const bool in1 = (t1 > lo && t1 < hi_), in2 = (t2 > lo && t2 < hi_);
                if (in1 && in2) eta = (fabs(e1) <= fabs(e2)) ? e1 : e2;
                else if (in1) eta = e1;
                else if (in2) eta = e2;
                else eta = 0.5 * (lo + hi_) - tau;
            }
            double tn = tau + eta;
            if (!(tn > lo && tn < hi_) || !(tn == tn)) tn = 0.5 * (lo + hi_);
            if (tn == tau) break;
            tau = tn;
        }
    }
    const double dorg = dn[org];
    const double lm = dorg + tau;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
        if (j < k) {
            double dl = (dnl[q] - dorg) - tau;
            // interlacing is what makes the Loewner product positive: enforce it against rounding
            if (j == i && dl >= 0.0) dl = -MG_TINY;
            if (j == i + 1 && dl <= 0.0) dl = MG_TINY;
            delta[(size_t)i * k + j] = dl;
        }
    }
    if (lane == 0) { lam[i] = lm; iters[i] = it; }
}

__global__ __launch_bounds__(256) void k_mg_weights(const double* __restrict__ pack, const double* __restrict__ delta,
                                                    double* __restrict__ zhat) {
#pragma clang fp contract(off)
    const int* hi = reinterpret_cast<const int*>(pack);
    const int k = hi[3];
    __shared__ double s_st[4][MG_LD];
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= k) return;
    double* st = s_st[threadIdx.x >> 6];
    const double* dn = pack + MG_DN;
    const double rho = pack[MG_SC];
    const double dj = dn[j];
    // prod_i (lam_i - dn_j) / prod_{i != j} (dn_i - dn_j), paired so that every ratio is positive: the ratios on the
    // lanes, the product in the host's order on lane 0
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        if (i < k - 1) st[i] = delta[(size_t)i * k + j] / (dj - dn[i < j ? i : i + 1]);
    }
    mg_stage_sync();
    if (lane == 0) {
        double prod = -delta[(size_t)(k - 1) * k + j];                  // lam_{k-1} - dn_j > 0
#pragma unroll 8
        for (int i = 0; i < k - 1; ++i) prod *= st[i];
        const double v = sqrt(fabs(prod) / rho);
        zhat[j] = pack[MG_ZN + j] < 0.0 ? -v : v;
    }
}

__global__ __launch_bounds__(256) void k_mg_vectors(const double* __restrict__ pack, const double* __restrict__ Qf,
                                                    const double* __restrict__ lam, const double* __restrict__ delta,
                                                    const double* __restrict__ zhat, const int* __restrict__ iters,
                                                    double* __restrict__ S, double* __restrict__ rec, int* __restrict__ src) {
#pragma clang fp contract(off)
    const int* hi = reinterpret_cast<const int*>(pack);
    const int K = hi[0], k = hi[3];
    __shared__ double s_st[4][MG_LD];
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);       // eigenvalue of T: root t, or deflated pole df[t - k]
    if (t >= K) return;
    double* st = s_st[threadIdx.x >> 6];
    const int* nd = hi + MG_I_ND;
    const int* df = hi + MG_I_DF;
    const double* d = pack + MG_D;
    double v, e;
    if (t < k) {
        double s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q;
            s[q] = j < k ? zhat[j] / delta[(size_t)t * k + j] : 0.0;
            if (j < k) st[j] = s[q] * s[q];
        }
        mg_stage_sync();
        double nn = lane == 0 ? mg_serial_sum(st, 0, k) : 0.0;
        mg_stage_sync();
        nn = mg_from_lane<0>(nn);
        const double inv = 1.0 / sqrt(nn);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q;
            if (j < k) {
                s[q] *= inv;
                S[(size_t)t * k + j] = s[q];
                st[j] = Qf[(size_t)nd[j] * K + (K - 1)] * s[q];
            }
        }
        mg_stage_sync();
        e = lane == 0 ? mg_serial_sum(st, 0, k) : 0.0;
        mg_stage_sync();
        e = mg_from_lane<0>(e);
        v = lam[t];
    } else {
        const int p = df[t - k];
        v = d[p];
        e = Qf[(size_t)p * K + (K - 1)];
    }
    // ascending position = how many come before in (value, list order): the host's stable_sort
    int cnt = 0;
    for (int u = lane; u < K; u += 64) {
        const double vu = u < k ? lam[u] : d[df[u - k]];
        cnt += (vu < v || (vu == v && u < t)) ? 1 : 0;
    }
    cnt = mg_wave_count(cnt);
    if (lane == 0) {
        const int c = K - 1 - cnt;                           // :LR -> descending
        rec[c] = pack[MG_SC + 1] * e;
        rec[MAXK + c] = v;
        src[c] = t;
    }
    if (t == 0) {                                            // status: roots at the iteration cap or not finite
        int bad = 0;
        for (int u = lane; u < k; u += 64) bad += (iters[u] >= 80 || !(fabs(lam[u]) <= 1.7976931348623157e308)) ? 1 : 0;
        bad = mg_wave_count(bad);
        if (lane == 0) rec[2 * MAXK] = (double)bad;
    }
}

__global__ __launch_bounds__(256) void k_mg_eigvecs(const double* __restrict__ pack, const double* __restrict__ Qf,
                                                    const double* __restrict__ S, const int* __restrict__ src,
                                                    double* __restrict__ Uall) {
#pragma clang fp contract(off)
    __shared__ double s_s[MG_LD];
    __shared__ int s_nd[MG_LD];
    const int* hi = reinterpret_cast<const int*>(pack);
    const int K = hi[0], k = hi[3];
    const int c = blockIdx.x, r = threadIdx.x;
    const int t = src[c];
    if (t >= k) {                                            // deflated pole: its column of Qf as it stands
        if (r < K) Uall[(size_t)c * K + r] = Qf[(size_t)hi[MG_I_DF + (t - k)] * K + r];
        return;
    }
    if (r < k) { s_s[r] = S[(size_t)t * k + r]; s_nd[r] = hi[MG_I_ND + r]; }
    __syncthreads();
    if (r >= K) return;
    // The host's product (Rank1Merge::vectors) runs its blocks of eight rows of either row panel through an FMA kernel and
    // the remaining rows through a multiply-add loop, both in pole order; the columns it skips are exact zeros here.
    const int k1 = hi[1], k2 = hi[2];
    const bool fused = hi[6] != 0 && (r < k1 ? r < (k1 & ~7) : r - k1 < (k2 & ~7));
    // (eight loads in flight per row: one at a time this product is a chain of k memory latencies)
    double acc = 0.0;
    int j = 0;
    for (; j + 8 <= k; j += 8) {
        double q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = Qf[(size_t)s_nd[j + u] * K + r];
        if (fused) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fma(q[u], s_s[j + u], acc);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += q[u] * s_s[j + u];
        }
    }
    for (; j < k; ++j) {
        const double q = Qf[(size_t)s_nd[j] * K + r];
        if (fused) acc = fma(q, s_s[j], acc); else acc += q * s_s[j];
    }
    Uall[(size_t)c * K + r] = acc;
}

}  // namespace dev

// Buffers and launches of one workspace's device merge.  Shared by the Lanczos driver (Solver::lz_device_merge) and the
// test entry proxsdp_device_symeig_split: both go through stage_first() and run().
struct DeviceMerge {
    DevBuf<double> Q1d, pack_d, Qf, lam, delta, zhat, S, rec_d, Uall;
    DevBuf<int> iters_d, src_d;
    PinnedBuf q1_h, pack_h, rec_h;
    Event ev_q1, ev_rec;
    bool ready = false;
    int K = 0, k = 0, ndf = 0;                               // of the last run()
    void ensure() {
        if (ready) return;
        const size_t kk = (size_t)dev::MG_KMAX * dev::MG_KMAX;
        Q1d.alloc(kk); pack_d.alloc(dev::MG_PACK); Qf.alloc(kk); lam.alloc(dev::MG_LD); delta.alloc(kk); zhat.alloc(dev::MG_LD);
        S.alloc(kk); rec_d.alloc(dev::MG_REC); Uall.alloc(kk);
        iters_d.alloc(dev::MG_LD); src_d.alloc(dev::MG_LD);
        q1_h.alloc(kk); pack_h.alloc(dev::MG_PACK); rec_h.alloc(dev::MG_REC);
        ev_q1.create(hipEventDisableTiming); ev_rec.create(hipEventDisableTiming);
        ready = true;
    }
    static bool eligible(int K) { return K >= 2 && K <= dev::MG_KMAX; }
    // Q1 of the split's first part to the device on `side` (hidden under the rest of the cycle); run() waits on the event
    void stage_first(const SplitEig& Sp, hipStream_t side) {
        ensure();
        const size_t n1 = (size_t)Sp.k1 * Sp.k1;
        if (Sp.k1 < 1 || Sp.k1 >= dev::MG_KMAX) throw std::logic_error("device merge: first part too large");
        std::memcpy(q1_h.p, Sp.Q1.data(), n1 * sizeof(double));
        PX_HIP(hipMemcpyAsync(Q1d.p, q1_h.p, n1 * sizeof(double), hipMemcpyHostToDevice, side));
        PX_HIP(hipEventRecord(ev_q1, side));
    }
    // The merge of Sp (first part staged, tail decomposed: Sp.Q2 / d2) on `stream`: plan without Qf, one packed upload,
    // four launches, the record's copy, the eigenvector launch.  wait(event) blocks until the record has landed.
    // Returns false when the host has to redo this merge (a root hit the iteration cap, a non-finite value): D / f are
    // then untouched.  On success D[c], f[c] (c < K, descending) are filled and Uall holds the K columns.
    template <typename Wait>
    bool run(SplitEig& Sp, int K_, double betaK, hipStream_t stream, Wait&& wait, double* D, double* f) {
        ensure();
        Rank1Merge& M = Sp.M;
        const int k1 = Sp.k1, k2 = K_ - k1;
        if (!eligible(K_) || k1 < 1 || k2 < 1) return false;
        M.plan(k1, k2, Sp.Q1.data(), Sp.d1.data(), Sp.Q2.data(), Sp.d2.data(), Sp.beta, false);
        K = K_; k = M.k; ndf = (int)M.df.size();
        const int nrot = (int)M.rots.size();
        if (k + ndf != K || nrot >= dev::MG_LD) throw std::logic_error("device merge: inconsistent plan");
        int* hi = reinterpret_cast<int*>(pack_h.p);
        hi[0] = K; hi[1] = k1; hi[2] = k2; hi[3] = k; hi[4] = ndf; hi[5] = nrot; hi[6] = rank1_panel_uses_fma() ? 1 : 0; hi[7] = 0;
        for (int p = 0; p < K; ++p) hi[dev::MG_I_COLSRC + p] = M.colsrc[p];
        for (int j = 0; j < k; ++j) hi[dev::MG_I_ND + j] = M.nd[j];
        for (int j = 0; j < ndf; ++j) hi[dev::MG_I_DF + j] = M.df[j];
        double* pd = pack_h.p;
        pd[dev::MG_SC] = M.rho; pd[dev::MG_SC + 1] = betaK;
        for (int q = 0; q < nrot; ++q) {
            hi[dev::MG_I_RPJ + q] = M.rots[q].pj; hi[dev::MG_I_RJ + q] = M.rots[q].j;
            pd[dev::MG_RC + q] = M.rots[q].c; pd[dev::MG_RS + q] = M.rots[q].s;
        }
        for (int p = 0; p < K; ++p) pd[dev::MG_D + p] = M.d[p];
        for (int j = 0; j < k; ++j) { pd[dev::MG_DN + j] = M.dn[j]; pd[dev::MG_ZN + j] = M.zn[j]; }
        std::memcpy(pd + dev::MG_Q2, Sp.Q2.data(), (size_t)k2 * k2 * sizeof(double));
        PX_HIP(hipMemcpyAsync(pack_d.p, pack_h.p, ((size_t)dev::MG_Q2 + (size_t)k2 * k2) * sizeof(double), hipMemcpyHostToDevice, stream));
        PX_HIP(hipStreamWaitEvent(stream, ev_q1, 0));
        const double* pk = pack_d.p;
        hipLaunchKernelGGL(dev::k_mg_roots, dim3((k + 3) / 4 + K), dim3(256), 0, stream, pk, (const double*)Q1d.p, Qf.p, lam.p,
                           delta.p, iters_d.p);
        if (nrot > 0) hipLaunchKernelGGL(dev::k_mg_rotate, dim3((K + 63) / 64), dim3(64), 0, stream, pk, Qf.p);
        if (k > 0) hipLaunchKernelGGL(dev::k_mg_weights, dim3((k + 3) / 4), dim3(256), 0, stream, pk, (const double*)delta.p, zhat.p);
        hipLaunchKernelGGL(dev::k_mg_vectors, dim3((K + 3) / 4), dim3(256), 0, stream, pk, (const double*)Qf.p, (const double*)lam.p,
                           (const double*)delta.p, (const double*)zhat.p, (const int*)iters_d.p, S.p, rec_d.p, src_d.p);
        PX_HIP(hipMemcpyAsync(rec_h.p, rec_d.p, dev::MG_REC * sizeof(double), hipMemcpyDeviceToHost, stream));
        PX_HIP(hipEventRecord(ev_rec, stream));
        hipLaunchKernelGGL(dev::k_mg_eigvecs, dim3(K), dim3(256), 0, stream, pk, (const double*)Qf.p, (const double*)S.p,
                           (const int*)src_d.p, Uall.p);
        PX_HIP(hipGetLastError());
        wait((hipEvent_t)ev_rec);
        const double* r = rec_h.p;
        bool ok = (r[2 * dev::MAXK] == 0.0);
        for (int c = 0; ok && c < K; ++c) ok = std::isfinite(r[c]) && std::isfinite(r[dev::MAXK + c]);
        if (!ok) return false;
        for (int c = 0; c < K; ++c) { f[c] = r[c]; D[c] = r[dev::MAXK + c]; }
        return true;
    }
};

}  // namespace proxsdp
