// The step of a cutting-plane loop after the triangles (triangle_cuts.hip.hpp): GROW given bases -- triangles into pentagons,
// pentagons into heptagons -- by the most violated pair of further nodes and signs (proxsdp_hip_model_cliques, host restatement
// proxsdp_host_clique_cuts; the contract is in include/proxsdp_hip.h).  No line of the reference stands behind this file.
//
// Value.  For a base a_0 < ... < a_{q-1} with signs sigma, nodes l < m outside it and tau_l, tau_m = +-1
//     v = (((B - tau_l t_l) - tau_m t_m) - (tau_l tau_m) X[l, m]) - rhs        fp64, this association, contraction off
// with t_l = sum_u sigma_u X[a_u, l] and B the base's own pair sum.  The best extension of a base is the maximum of v under
// the total order (v descending, then (l, m, code) ascending): clique_better of clique_cuts_host.hpp, with (l, m, code) as
// the one number key = (l s + m) 4 + code.
//
// Device.  dense_cone_matrix (model_call.hip.hpp) builds the dense X.  Bases go through in batches of CLQ_WAVE-multiples so that t stays bounded:
// k_clique_rows writes t[l][b] (the base is the fast index; NaN at a base's own nodes, and in the columns that pad a batch to
// whole waves, so that no comparison passes there and the sweep needs no membership test) and B[b].  k_clique_sweep: a
// workgroup of 4 waves owns 64 bases, one per lane, and a range of 64 x 64 tiles of (l, m) pairs of the strict upper triangle;
// per tile X[l, m] is staged in LDS with NaN at l >= m and past the side and read as a broadcast, t_m is staged as [m][lane]
// (conflict-free), t_l comes from global memory once per l (coalesced, one load per 64 pairs); the wave with number w takes the
// rows l = w, w + 4, ... of the tile.  Each lane evaluates the four codes in order and keeps its best (v, key) in registers
// under the total order: no cross-lane traffic inside a tile.  64 KiB of LDS: two workgroups per CU.  The four waves' bests
// are merged through LDS and the workgroup writes ONE partial per (its tile range, base); k_clique_best reduces the partials of
// a base.  The maximum under a total order does not depend on how the pairs were split: grid and batch are invisible.
// The host half -- checks, order, serial restatement, normal form, merge, sort, rows -- is clique_cuts_host.hpp.
#pragma once
#include "model_call.hip.hpp"
#include "clique_cuts_host.hpp"

namespace proxsdp {

constexpr int CLQ_TILE = 64;                    // side of a tile of (l, m) pairs
constexpr int CLQ_WAVE = 64;                    // bases of a workgroup of the sweep: one per lane

namespace dev {

#pragma clang fp contract(off)
// grid: x = chunks of CLQ_TILE values of l, y = groups of CLQ_WAVE bases of the batch.  nodes / sign: nb x Q, the batch's
// bases.  t: s x bp (bp = the batch rounded up to whole waves), Bv: bp
template <int Q>
__global__ void __launch_bounds__(TPB)
k_clique_rows(const double* __restrict__ X, int s, const int* __restrict__ nodes, const signed char* __restrict__ sign, int nb,
              int bp, double* __restrict__ t, double* __restrict__ Bv) {
    __shared__ double tile[CLQ_WAVE][CLQ_TILE + 1];                 // [base][l]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l0 = (int)blockIdx.x * CLQ_TILE, b0 = (int)blockIdx.y * CLQ_WAVE;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int l = l0 + lane;
    for (int bb = w; bb < CLQ_WAVE; bb += NWAVE) {                  // a wave reads the Q rows X[a_u, l0 ...] contiguously
        const int b = b0 + bb;
        double acc = nan;
        if (b < nb && l < s) {
            bool own = false;
            double a = 0.0;
#pragma unroll
            for (int u = 0; u < Q; ++u) {
                const int au = nodes[b * Q + u];
                const double term = (double)sign[b * Q + u] * X[(long long)au * s + l];
                a = u == 0 ? term : a + term;
                own = own || au == l;
            }
            acc = own ? nan : a;
        }
        tile[bb][lane] = acc;
    }
    __syncthreads();
    for (int r = w; r < CLQ_TILE; r += NWAVE)                       // and writes t along the bases
        if (l0 + r < s) t[(long long)(l0 + r) * bp + b0 + lane] = tile[lane][r];
    if (blockIdx.x == 0 && tid < CLQ_WAVE) {
        const int b = b0 + tid;
        double B = nan;
        if (b < nb) {
            bool first = true;
#pragma unroll
            for (int u = 0; u < Q; ++u)
#pragma unroll
                for (int v = u + 1; v < Q; ++v) {
                    const double sg = (double)(-(int)sign[b * Q + u] * (int)sign[b * Q + v]);
                    const double term = sg * X[(long long)nodes[b * Q + u] * s + nodes[b * Q + v]];
                    B = first ? term : B + term;
                    first = false;
                }
        }
        Bv[b] = B;
    }
}

// grid: x = workgroup columns, each with the tiles [x NT / gridDim.x, (x + 1) NT / gridDim.x) of the NT = nt (nt + 1) / 2
// tiles (block row <= block column, column by column); y = groups of CLQ_WAVE bases.  part: gridDim.x x bp
__global__ void __launch_bounds__(TPB)
k_clique_sweep(const double* __restrict__ X, int s, int nt, const double* __restrict__ t, const double* __restrict__ Bv, int bp,
               double rhs, CliqueBest* __restrict__ part) {
    __shared__ double XT[CLQ_TILE][CLQ_TILE];                       // [l][m], NaN where l >= m or m is past the side
    __shared__ double TM[CLQ_TILE][CLQ_WAVE];                       // [m][base]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = (int)blockIdx.y * CLQ_WAVE + lane;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const long long NT = (long long)nt * (nt + 1) / 2;
    const int T0 = (int)((long long)blockIdx.x * NT / gridDim.x), T1 = (int)((long long)(blockIdx.x + 1) * NT / gridDim.x);
    int bj = (int)((sqrtf(8.0f * (float)T0 + 1.0f) - 1.0f) * 0.5f);
    while ((bj + 1) * (bj + 2) / 2 <= T0) ++bj;
    while (bj * (bj + 1) / 2 > T0) --bj;
    int bi = T0 - bj * (bj + 1) / 2;
    const double Bb = Bv[b];
    double bv = -__longlong_as_double(0x7ff0000000000000ll);        // -infinity
    unsigned long long bkey = CLQ_NO_KEY;
    for (int T = T0; T < T1; ++T) {
        const int L0 = bi * CLQ_TILE, M0 = bj * CLQ_TILE;
        __syncthreads();                                            // the previous tile is done with the staging
#pragma unroll 4
        for (int r = w; r < CLQ_TILE; r += NWAVE) {
            const int l = L0 + r, m = M0 + lane;
            XT[r][lane] = (l < m && m < s) ? X[(long long)l * s + m] : nan;
            const int mr = M0 + r;
            TM[r][lane] = mr < s ? t[(long long)mr * bp + b] : nan;
        }
        __syncthreads();
        const int lend = s - L0 < CLQ_TILE ? s - L0 : CLQ_TILE;
        double tl_next = w < lend ? t[(long long)(L0 + w) * bp + b] : nan;
        for (int li = w; li < lend; li += NWAVE) {
            const double tl = tl_next;
            if (li + NWAVE < lend) tl_next = t[(long long)(L0 + li + NWAVE) * bp + b];
            const double p = Bb - tl, n = Bb + tl;                  // B - tau_l t_l for tau_l = +1, -1
            const int m0 = bi == bj ? li + 1 : 0;                   // (below the diagonal of a diagonal tile: NaN anyway)
            const unsigned long long krow = ((unsigned long long)(L0 + li) * (unsigned long long)s + (unsigned long long)M0) * 4ull;
#pragma unroll 4
            for (int mi = m0; mi < CLQ_TILE; ++mi) {
                const double x = XT[li][mi], tm = TM[mi][lane];
                const double v0 = ((p - tm) - x) - rhs;
                const double v1 = ((p + tm) + x) - rhs;
                const double v2 = ((n - tm) + x) - rhs;
                const double v3 = ((n + tm) - x) - rhs;
                const double vm = fmax(fmax(v0, v1), fmax(v2, v3)); // (a NaN operand makes all four NaN: vm is NaN then)
                if (vm >= bv) {
                    const unsigned long long key = krow + 4ull * (unsigned long long)mi;
                    if (clique_better(v0, key, bv, bkey)) { bv = v0; bkey = key; }
                    if (clique_better(v1, key + 1, bv, bkey)) { bv = v1; bkey = key + 1; }
                    if (clique_better(v2, key + 2, bv, bkey)) { bv = v2; bkey = key + 2; }
                    if (clique_better(v3, key + 3, bv, bkey)) { bv = v3; bkey = key + 3; }
                }
            }
        }
        if (++bi > bj) { bi = 0; ++bj; }
    }
    // the four waves' bests of a base into one
    __syncthreads();
    double* rv = &XT[0][0];
    unsigned long long* rk = reinterpret_cast<unsigned long long*>(&TM[0][0]);
    rv[w * CLQ_WAVE + lane] = bv;
    rk[w * CLQ_WAVE + lane] = bkey;
    __syncthreads();
    if (w == 0) {
        for (int o = 1; o < NWAVE; ++o) {
            const double v = rv[o * CLQ_WAVE + lane];
            const unsigned long long key = rk[o * CLQ_WAVE + lane];
            if (clique_better(v, key, bv, bkey)) { bv = v; bkey = key; }
        }
        CliqueBest out;
        out.v = bv; out.key = bkey;
        part[(long long)blockIdx.x * bp + b] = out;
    }
}
#pragma clang fp contract(fast)

// best[b] = the maximum of part[0 .. gx)[b] under the total order
__global__ void __launch_bounds__(TPB)
k_clique_best(const CliqueBest* __restrict__ part, int gx, int bp, CliqueBest* __restrict__ best) {
    const int b = (int)blockIdx.x * TPB + threadIdx.x;
    if (b >= bp) return;
    CliqueBest r = part[b];
    for (int g = 1; g < gx; ++g) {
        const CliqueBest c = part[(long long)g * bp + b];
        if (clique_better(c.v, c.key, r.v, r.key)) r = c;
    }
    best[b] = r;
}

}  // namespace dev

// proxsdp_hip_model_cliques on the model's stream.  ord_h / ord_d: the cone's variable list (0-based caller numbers) on the
// host and on the device; q: checked by check_clique_struct and check_clique_bases
inline void device_clique_cuts(hipStream_t st, const int64_t* ord_h, const long long* ord_d, int64_t s, int base, int cone,
                               proxsdp_clique_cuts& q) {
    const double t0 = now_s();
    AllocCount counting;
    const int bq = q.base_size;
    const DevBuf<double> X = dense_cone_matrix(st, q.primal, q.on_device != 0, ord_h, ord_d, s,
                                               "proxsdp_clique_cuts: non-finite entry of primal in cone " + std::to_string(cone));
    // the launch: bp bases per batch in whole waves, gx workgroup columns over the NT tiles
    const int64_t want = q.batch > 0 ? q.batch : CLQ_DEFAULT_BATCH;
    const int bp = (int)((std::min<int64_t>(want, q.n_base) + CLQ_WAVE - 1) / CLQ_WAVE * CLQ_WAVE);
    const int nt = (int)((s + CLQ_TILE - 1) / CLQ_TILE);
    const long long NT = (long long)nt * (nt + 1) / 2;
    const int groups = bp / CLQ_WAVE;
    const int gx = (int)std::min<long long>(NT, q.grid > 0 ? q.grid : std::max(1, 4096 / groups));
    DevBuf<double> t((size_t)s * (size_t)bp), Bv((size_t)bp);
    DevBuf<int> nodes_d((size_t)bp * (size_t)bq);
    DevBuf<signed char> sign_d((size_t)bp * (size_t)bq);
    DevBuf<CliqueBest> part((size_t)gx * (size_t)bp), best_d((size_t)bp);
    std::vector<CliqueBest> best((size_t)q.n_base);
    std::vector<int> nodes_h((size_t)bp * (size_t)bq);
    StreamTimer sweeps(st);
    for (int64_t b0 = 0; b0 < q.n_base; b0 += bp) {
        const int nb = (int)std::min<int64_t>(bp, q.n_base - b0);
        for (int64_t e = 0; e < (int64_t)nb * bq; ++e) nodes_h[(size_t)e] = (int)q.base_nodes[b0 * bq + e];
        nodes_d.upload(nodes_h.data(), (size_t)nb * (size_t)bq, st);
        sign_d.upload(reinterpret_cast<const signed char*>(q.base_sign + b0 * bq), (size_t)nb * (size_t)bq, st);
        const dim3 grid_rows((unsigned)nt, (unsigned)groups);
        if (bq == 3)
            hipLaunchKernelGGL(dev::k_clique_rows<3>, grid_rows, dim3(dev::TPB), 0, st, (const double*)X.p, (int)s,
                               (const int*)nodes_d.p, (const signed char*)sign_d.p, nb, bp, t.p, Bv.p);
        else
            hipLaunchKernelGGL(dev::k_clique_rows<5>, grid_rows, dim3(dev::TPB), 0, st, (const double*)X.p, (int)s,
                               (const int*)nodes_d.p, (const signed char*)sign_d.p, nb, bp, t.p, Bv.p);
        PX_HIP(hipGetLastError());
        sweeps.start();
        hipLaunchKernelGGL(dev::k_clique_sweep, dim3((unsigned)gx, (unsigned)groups), dim3(dev::TPB), 0, st, (const double*)X.p,
                           (int)s, nt, (const double*)t.p, (const double*)Bv.p, bp, q.rhs, part.p);
        PX_HIP(hipGetLastError());
        sweeps.stop();
        hipLaunchKernelGGL(dev::k_clique_best, dim3((unsigned)ceil_div(bp, dev::TPB)), dim3(dev::TPB), 0, st,
                           (const CliqueBest*)part.p, gx, bp, best_d.p);
        PX_HIP(hipGetLastError());
        best_d.download(best.data() + b0, (size_t)nb, st);
        PX_HIP(hipStreamSynchronize(st));                           // (the next batch overwrites the bases and t)
    }
    clique_write_rows(best, s, q, [&](int64_t i, int64_t j) { return ord_h[j * (j + 1) / 2 + i] + base; });
    q.sweep_seconds = sweeps.seconds();
    q.bytes_allocated = counting.bytes;
    q.seconds = now_s() - t0;
}

}  // namespace proxsdp
