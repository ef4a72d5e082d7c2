// A feasible point from a kept model: randomised hyperplane rounding of a PSD cone's factors to `trials` +-1 vectors at once
// and a one-flip local search against the objective the handle holds (proxsdp_hip_model_round; the contract, expression by
// expression, is in include/proxsdp_hip.h "rounding on a model handle"; host restatement proxsdp_host_round).  No line of the
// reference stands behind this file: ProxSDP returns the matrix only.
//
// Everything is bit-parallel over the trials: lane = trial, and the signs of 64 trials at one node are one 64-bit word (bit
// set: sigma = -1), words[i][T / 64].
//   k_round_adj_count / _fill  the adjacency of the cone's part of the exit path's unscaled c (xd.c: solver order, the cone's
//                       entries contiguous, upper triangle column by column): a wave per node walks j = 0 .. s-1 in pieces of
//                       64 -- column i above the diagonal, row i beyond it -- and compacts the non-zeros by ballot, so a
//                       node's neighbours ascend.  Between the two the s counts visit the host for the prefix sum; the values
//                       do not.
//   k_round_directions  g (r x T) from the integer generator: the bits are round_direction's (rounding_host.hpp)
//   k_round_signs       a workgroup owns 16 nodes and 4 words (a wave each); V[i, k] * w_k of a chunk of 64 columns is staged
//                       in LDS and read as broadcasts, each lane adds its trial's y in the order of k, and one ballot of
//                       y < 0 per node is the word
//   k_round_search      one wave owns a word column: value, sweeps, value again (round_pass).  The adjacency of node i is
//                       wave-uniform: the wave loads it once, 64 entries a time and a node ahead, and hands it round by
//                       v_readlane; each lane extracts its bit of words[j], the flips of node i are the ballot of
//                       sigma_i a > 0, XORed into the word.  Every lane stores the (uniform) new word, so each lane reads
//                       back what it wrote itself and no barrier stands inside a sweep.  A lane whose sweep flipped nothing is at its fixed point
//                       and flips nothing later, so the wave runs until its ballot of "flipped this sweep" is empty and each
//                       trial ends where its own loop would.  The column lives in LDS (IN_LDS, s <= lds_side) or in the
//                       wave's slice of `cols` in global memory; either way the final column is left in `cols`, contiguous,
//                       for the one download of the best trial.
// Every kernel grid-strides over its work items, and nothing is accumulated across items: the result does not depend on
// the launch.  The host half -- checks, weights, generator, best trial, serial restatement -- is rounding_host.hpp.
#pragma once
#include "model_call.hip.hpp"
#include "rounding_host.hpp"

namespace proxsdp {

constexpr int ROUND_NI = 16;                    // nodes of a workgroup of k_round_signs
constexpr int ROUND_KC = 64;                    // columns of V staged at a time

namespace dev {

#pragma clang fp contract(off)
__device__ __forceinline__ unsigned long long round_mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double round_u53(unsigned long long seed, unsigned long long counter) {
    const unsigned long long key = seed ^ ((counter + 1ull) * 0xD1342543DE82EF95ull);
    return (double)(round_mix(key) >> 11) * (1.0 / 9007199254740992.0);
}

// g[k T + t]
__global__ void __launch_bounds__(TPB)
k_round_directions(unsigned long long seed, int r, int T, double* __restrict__ g) {
    const long long total = (long long)r * T, stride = (long long)gridDim.x * TPB;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += stride) {
        const long long k = e / T, t = e - k * T;
        const unsigned long long base = ((unsigned long long)t * (unsigned long long)r + (unsigned long long)k) * 12ull;
        double z = round_u53(seed, base);
#pragma unroll
        for (int q = 1; q < 12; ++q) z = z + round_u53(seed, base + (unsigned long long)q);
        g[e] = z - 6.0;
    }
}

// the cone's entry of (i, j), i != j
__device__ __forceinline__ long long round_tri(int i, int j) {
    return j < i ? (long long)i * (i + 1) / 2 + j : (long long)j * (j + 1) / 2 + i;
}

// cnt[i] = number of j != i with cc(i, j) != 0; diag[i] = cc(i, i).  A wave per node.
__global__ void __launch_bounds__(TPB)
k_round_adj_count(const double* __restrict__ cc, int s, int* __restrict__ cnt, double* __restrict__ diag) {
    const int lane = threadIdx.x & 63, nw = (int)gridDim.x * NWAVE;
    for (int i = (int)blockIdx.x * NWAVE + (threadIdx.x >> 6); i < s; i += nw) {
        int c = 0;
        for (int j0 = 0; j0 < s; j0 += 64) {
            const int j = j0 + lane;
            const bool nz = j < s && j != i && cc[round_tri(i, j)] != 0.0;
            c += __popcll(__ballot(nz));
        }
        if (lane == 0) { cnt[i] = c; diag[i] = cc[(long long)i * (i + 1) / 2 + i]; }
    }
}

// node i's neighbours, ascending, at ptr[i]: a piece's non-zeros are ranked by the ballot, the pieces follow each other
__global__ void __launch_bounds__(TPB)
k_round_adj_fill(const double* __restrict__ cc, int s, const long long* __restrict__ ptr, int* __restrict__ col,
                 double* __restrict__ val) {
    const int lane = threadIdx.x & 63, nw = (int)gridDim.x * NWAVE;
    for (int i = (int)blockIdx.x * NWAVE + (threadIdx.x >> 6); i < s; i += nw) {
        long long at = ptr[i];
        for (int j0 = 0; j0 < s; j0 += 64) {
            const int j = j0 + lane;
            const double w = (j < s && j != i) ? cc[round_tri(i, j)] : 0.0;
            const unsigned long long bal = __ballot(w != 0.0);
            if (w != 0.0) {
                const long long pos = at + __popcll(bal & (((unsigned long long)1 << lane) - 1));
                col[pos] = j; val[pos] = w;
            }
            at += __popcll(bal);
        }
    }
}

// words[i nwords + tw] = the ballot over the 64 trials of word tw of y(i, t) < 0.  Work items: (tile of ROUND_NI nodes,
// group of NWAVE words), walked by the workgroups; wave wv of a workgroup takes word 4 grp + wv
__global__ void __launch_bounds__(TPB)
k_round_signs(const double* __restrict__ V, const double* __restrict__ w, const double* __restrict__ g, int s, int r, int T,
              unsigned long long* __restrict__ words) {
    __shared__ double a[ROUND_KC][ROUND_NI];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nwords = T / 64, ntile = (s + ROUND_NI - 1) / ROUND_NI, ngrp = (nwords + NWAVE - 1) / NWAVE;
    const long long items = (long long)ntile * ngrp;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int tile = (int)(item % ntile), grp = (int)(item / ntile);
        const int i0 = tile * ROUND_NI, tw = grp * NWAVE + wv;
        const bool live = tw < nwords;                              // (wave-uniform)
        double y[ROUND_NI];
#pragma unroll
        for (int ii = 0; ii < ROUND_NI; ++ii) y[ii] = 0.0;
        for (int kc = 0; kc < r; kc += ROUND_KC) {
            __syncthreads();                                        // the previous chunk, or item, is done with the tile
#pragma unroll
            for (int q = 0; q < ROUND_KC * ROUND_NI / TPB; ++q) {
                const int kk = (tid >> 4) + (TPB / ROUND_NI) * q, ii = tid & (ROUND_NI - 1);
                const int k = kc + kk, i = i0 + ii;
                a[kk][ii] = (k < r && i < s) ? V[(long long)k * s + i] * w[k] : 0.0;
            }
            __syncthreads();
            if (live) {
                const int kn = r - kc < ROUND_KC ? r - kc : ROUND_KC;
                const double* gp = g + (long long)kc * T + (long long)tw * 64 + lane;
                for (int kk = 0; kk < kn; ++kk) {
                    const double gk = gp[(long long)kk * T];
#pragma unroll
                    for (int ii = 0; ii < ROUND_NI; ++ii) y[ii] = y[ii] + a[kk][ii] * gk;
                }
            }
        }
        if (live) {
#pragma unroll
            for (int ii = 0; ii < ROUND_NI; ++ii) {
                const unsigned long long bal = __ballot(y[ii] < 0.0);
                if (lane == 0 && i0 + ii < s) words[(long long)(i0 + ii) * nwords + tw] = bal;
            }
        }
    }
}

// a wave-uniform value out of lane q's register (q uniform: one v_readlane per 32 bits, no LDS)
__device__ __forceinline__ double round_lane_d(double v, int q) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), q), __builtin_amdgcn_readlane(__double2loint(v), q));
}
__device__ __forceinline__ long long round_lane_ll(long long v, int q) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, q);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), q);
    return (long long)(((unsigned long long)hi << 32) | (unsigned long long)lo);
}

// One walk over the nodes 0 .. s-1 of the lane's trial of a word column, in the contract's order.
//   SWEEP = false: returns the value f (the diagonal, then per node sigma_i times the sum over the neighbours j > i)
//   SWEEP = true:  one sweep of the search (per node the sum over all neighbours, the ballot of sigma_i a > 0 XORed into the
//                  node's word: every lane stores the same word); adds the flips to `flips`, returns non-zero when any lane flipped
// What is wave-uniform is fetched once by the wave and handed round with v_readlane: the offsets ptr[i + 1] and the diagonal of
// 64 nodes at a time, and a node's neighbours and weights 64 at a time, one per lane -- the NEXT node's while this one's sums
// run (its entries start where this node's end; what lies past its own end is loaded, inside the arrays, and not used), so no
// sum waits for a load of the adjacency.  nnz = ptr[s].
template <bool SWEEP>
__device__ __forceinline__ double round_pass(unsigned long long* col, int s, long long nnz, const long long* __restrict__ ptr,
                                             const int* __restrict__ acol, const double* __restrict__ aval,
                                             const double* __restrict__ diag, int lane, long long& flips) {
    double f = 0.0;
    if (!SWEEP)
        for (int i0 = 0; i0 < s; i0 += WAVE) {
            const double myd = i0 + lane < s ? diag[i0 + lane] : 0.0;
            const int ni = s - i0 < WAVE ? s - i0 : WAVE;
            for (int ii = 0; ii < ni; ++ii) f = f + round_lane_d(myd, ii);
        }
    bool any = false;
    long long e0 = 0;
    int nc = 0;
    double nw = 0.0;
    if (lane < nnz) { nc = acol[lane]; nw = aval[lane]; }
    for (int i0 = 0; i0 < s; i0 += WAVE) {
        const int ip = i0 + lane + 1;
        const long long mypn = ptr[ip <= s ? ip : s];
        const int ni = s - i0 < WAVE ? s - i0 : WAVE;
        for (int ii = 0; ii < ni; ++ii) {
            const int i = i0 + ii;
            const long long e1 = round_lane_ll(mypn, ii);
            int cc = nc;
            double cw = nw;
            if (e1 + lane < nnz) { nc = acol[e1 + lane]; nw = aval[e1 + lane]; }
            double a = 0.0;
            for (long long eb = e0;;) {
                const int cnt = e1 - eb < WAVE ? (int)(e1 - eb) : WAVE;
                for (int q = 0; q < cnt; ++q) {
                    const int j = __builtin_amdgcn_readlane(cc, q);
                    const double w = round_lane_d(cw, q);
                    if (SWEEP || j > i) a = a + w * (((col[j] >> lane) & 1ull) ? -1.0 : 1.0);
                }
                eb += WAVE;
                if (eb >= e1) break;
                cc = eb + lane < e1 ? acol[eb + lane] : 0;              // (a node of more than 64 neighbours: the next piece)
                cw = eb + lane < e1 ? aval[eb + lane] : 0.0;
            }
            const unsigned long long wi = col[i];
            const double si = ((wi >> lane) & 1ull) ? -1.0 : 1.0;
            if (SWEEP) {
                const unsigned long long fl = __ballot(si * a > 0.0);
                if (fl) {                                           // (uniform)
                    col[i] = wi ^ fl;
                    flips += __popcll(fl);
                    any = true;
                }
            } else {
                f = f + si * a;
            }
            e0 = e1;
        }
    }
    return SWEEP ? (any ? 1.0 : 0.0) : f;
}

// grid: any; a workgroup is ONE wave and walks the word columns tw = blockIdx.x, + gridDim.x, ...  IN_LDS: dynamic LDS of
// 8 s bytes.  Out: cols[tw s + i] = the final words; v_rounded / v_final [T]; wsweeps / wflips [T / 64] per word column
template <bool IN_LDS>
__global__ void __launch_bounds__(WAVE)
k_round_search(const unsigned long long* __restrict__ words, int s, int nwords, long long nnz, const long long* __restrict__ ptr,
               const int* __restrict__ acol, const double* __restrict__ aval, const double* __restrict__ diag, int max_sweeps,
               unsigned long long* cols, double* __restrict__ v_rounded, double* __restrict__ v_final,
               int* __restrict__ wsweeps, long long* __restrict__ wflips) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long round_col_lds[];
    const int lane = threadIdx.x;
    for (int tw = blockIdx.x; tw < nwords; tw += gridDim.x) {
        unsigned long long* gcol = cols + (long long)tw * s;
        unsigned long long* col = IN_LDS ? round_col_lds : gcol;
        __syncthreads();                                            // (the previous column has left the LDS)
        for (int i = lane; i < s; i += WAVE) col[i] = words[(long long)i * nwords + tw];
        __syncthreads();                                            // one wave: the lanes see each other's words
        int sweeps = 0;
        long long flips = 0;
        v_rounded[(long long)tw * 64 + lane] = round_pass<false>(col, s, nnz, ptr, acol, aval, diag, lane, flips);
        while (sweeps < max_sweeps) {
            ++sweeps;
            if (round_pass<true>(col, s, nnz, ptr, acol, aval, diag, lane, flips) == 0.0) break;
        }
        v_final[(long long)tw * 64 + lane] = round_pass<false>(col, s, nnz, ptr, acol, aval, diag, lane, flips);
        if (IN_LDS) {
            __syncthreads();
            for (int i = lane; i < s; i += WAVE) gcol[i] = col[i];
        }
        if (lane == 0) { wsweeps[tw] = sweeps; wflips[tw] = flips; }
    }
}
#pragma clang fp contract(fast)

}  // namespace dev

// proxsdp_hip_model_round on the model's stream.  cc_d: the cone's part of the exit path's c on the device (s (s + 1) / 2
// entries); q: checked by check_rounding_struct / check_rounding_factors; cone: for the messages
inline void device_round(hipStream_t st, const double* cc_d, int64_t s, int cone, proxsdp_rounding& q) {
    const double t0 = now_s();
    AllocCount counting;
    const int r = q.r, T = q.trials, nwords = T / 64;
    // ---- the factors: V on the device, the weights from host values
    DevBuf<double> Vbuf, w_d((size_t)r);
    const double* V_d = q.V;
    std::vector<double> vals((size_t)r);
    if (q.on_device) {
        DevBuf<int> flag(1);                                        // (the check's wait brings the values too)
        PX_HIP(hipMemcpyAsync(vals.data(), q.values, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, st));
        require_finite_device(st, flag, q.V, s * r, "proxsdp_rounding: non-finite entry in V (proxsdp_rounding, cone " + std::to_string(cone) + ")");
    } else {
        std::copy(q.values, q.values + r, vals.begin());
        Vbuf.alloc((size_t)(s * r));
        Vbuf.upload(q.V, (size_t)(s * r), st);
        V_d = Vbuf.p;
    }
    const std::vector<double> w = round_weights(vals.data(), r);
    w_d.upload(w.data(), (size_t)r, st);
    // ---- the adjacency
    const int ga = q.grid_adjacency > 0 ? q.grid_adjacency : (int)std::min<int64_t>((s + dev::NWAVE - 1) / dev::NWAVE, 2048);
    DevBuf<int> cnt((size_t)s);
    DevBuf<double> diag_d((size_t)s);
    DevBuf<long long> ptr_d((size_t)s + 1);
    hipLaunchKernelGGL(dev::k_round_adj_count, dim3(ga), dim3(dev::TPB), 0, st, cc_d, (int)s, cnt.p, diag_d.p);
    PX_HIP(hipGetLastError());
    std::vector<int> cnt_h((size_t)s);
    cnt.download(cnt_h.data(), (size_t)s, st);
    PX_HIP(hipStreamSynchronize(st));
    std::vector<long long> ptr_h((size_t)s + 1, 0);
    for (int64_t i = 0; i < s; ++i) ptr_h[(size_t)i + 1] = ptr_h[(size_t)i] + cnt_h[(size_t)i];
    const long long nnz = ptr_h[(size_t)s];
    if (q.adj_ptr && nnz > q.adj_cap) throw std::logic_error("proxsdp_rounding: the device and the host count the adjacency differently");
    ptr_d.upload(ptr_h.data(), (size_t)s + 1, st);
    DevBuf<int> acol((size_t)std::max<long long>(nnz, 1));
    DevBuf<double> aval((size_t)std::max<long long>(nnz, 1));
    hipLaunchKernelGGL(dev::k_round_adj_fill, dim3(ga), dim3(dev::TPB), 0, st, cc_d, (int)s, (const long long*)ptr_d.p, acol.p, aval.p);
    PX_HIP(hipGetLastError());
    // ---- directions, signs
    DevBuf<double> g((size_t)r * (size_t)T), vr((size_t)T), vf((size_t)T);
    DevBuf<unsigned long long> words((size_t)s * (size_t)nwords), cols((size_t)s * (size_t)nwords);
    DevBuf<int> wsweeps((size_t)nwords);
    DevBuf<long long> wflips((size_t)nwords);
    const int gd = q.grid_directions > 0 ? q.grid_directions : grid_for((long long)r * T);
    hipLaunchKernelGGL(dev::k_round_directions, dim3(gd), dim3(dev::TPB), 0, st, (unsigned long long)q.seed, r, T, g.p);
    const long long items = ((s + ROUND_NI - 1) / ROUND_NI) * (long long)((nwords + dev::NWAVE - 1) / dev::NWAVE);
    const int gs = q.grid_signs > 0 ? q.grid_signs : (int)std::min<long long>(items, 65536);
    hipLaunchKernelGGL(dev::k_round_signs, dim3(gs), dim3(dev::TPB), 0, st, V_d, (const double*)w_d.p, (const double*)g.p,
                       (int)s, r, T, words.p);
    PX_HIP(hipGetLastError());
    // ---- values, search, values
    const int lds_side = q.lds_side < 0 ? 0 : std::min(q.lds_side > 0 ? q.lds_side : ROUND_LDS_SIDE, ROUND_LDS_SIDE_MAX);
    const bool in_lds = s <= lds_side;
    const int gq = q.grid_search > 0 ? std::min(q.grid_search, nwords) : nwords;
    StreamTimer search(st);
    search.start();
    if (in_lds)
        hipLaunchKernelGGL(dev::k_round_search<true>, dim3(gq), dim3(dev::WAVE), (size_t)s * sizeof(unsigned long long), st,
                           (const unsigned long long*)words.p, (int)s, nwords, nnz, (const long long*)ptr_d.p, (const int*)acol.p,
                           (const double*)aval.p, (const double*)diag_d.p, (int)q.max_sweeps, cols.p, vr.p, vf.p, wsweeps.p, wflips.p);
    else
        hipLaunchKernelGGL(dev::k_round_search<false>, dim3(gq), dim3(dev::WAVE), 0, st,
                           (const unsigned long long*)words.p, (int)s, nwords, nnz, (const long long*)ptr_d.p, (const int*)acol.p,
                           (const double*)aval.p, (const double*)diag_d.p, (int)q.max_sweeps, cols.p, vr.p, vf.p, wsweeps.p, wflips.p);
    PX_HIP(hipGetLastError());
    search.stop();
    // ---- the best trial on the host, its column, the optional outputs
    std::vector<double> vr_h((size_t)T), vf_h((size_t)T);
    std::vector<int> sw_h((size_t)nwords);
    std::vector<long long> fl_h((size_t)nwords);
    vr.download(vr_h.data(), (size_t)T, st); vf.download(vf_h.data(), (size_t)T, st);
    wsweeps.download(sw_h.data(), (size_t)nwords, st); wflips.download(fl_h.data(), (size_t)nwords, st);
    PX_HIP(hipStreamSynchronize(st));
    const int64_t best = round_best(vf_h.data(), T);
    std::vector<unsigned long long> column((size_t)s);
    PX_HIP(hipMemcpyAsync(column.data(), cols.p + (size_t)(best / 64) * (size_t)s, (size_t)s * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    if (q.adj_ptr) {
        static_assert(sizeof(long long) == sizeof(int64_t), "the offsets are copied as they are");
        std::vector<int> col_h((size_t)nnz);
        if (nnz > 0) {
            PX_HIP(hipMemcpyAsync(col_h.data(), acol.p, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost, st));
            aval.download(q.adj_val, (size_t)nnz, st);
        }
        diag_d.download(q.diag, (size_t)s, st);
        PX_HIP(hipStreamSynchronize(st));
        for (int64_t i = 0; i <= s; ++i) q.adj_ptr[i] = ptr_h[(size_t)i];
        for (long long e = 0; e < nnz; ++e) q.adj_col[e] = col_h[(size_t)e];
        q.adj_nnz = nnz;
    }
    PX_HIP(hipStreamSynchronize(st));
    const int bit = (int)(best % 64);
    for (int64_t i = 0; i < s; ++i) q.signs[i] = ((column[(size_t)i] >> bit) & 1ull) ? (int8_t)-1 : (int8_t)1;
    if (q.values_rounded) std::copy(vr_h.begin(), vr_h.end(), q.values_rounded);
    if (q.values_final) std::copy(vf_h.begin(), vf_h.end(), q.values_final);
    q.best_trial = best; q.value = vf_h[(size_t)best]; q.value_rounded = vr_h[(size_t)round_best(vr_h.data(), T)];
    q.flips = 0; q.sweeps = 0;
    for (int tw = 0; tw < nwords; ++tw) { q.flips += fl_h[(size_t)tw]; q.sweeps = std::max<int32_t>(q.sweeps, sw_h[(size_t)tw]); }
    q.search_seconds = search.seconds();
    q.bytes_allocated = counting.bytes;
    q.seconds = now_s() - t0;
}

}  // namespace proxsdp
