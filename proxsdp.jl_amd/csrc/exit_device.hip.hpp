// The exit path on the device (proxsdp_hip_solve_device; include/proxsdp_hip.h): what Solver::cache_solution and
// Solver::dual_feas_host (pdhg_loop.hip.hpp) compute -- get_duals + dual_feas + cone_feas + cache_solution, pdhg.jl:678-787 --
// without the iterate visiting the host.  The host sees the scalars, the 1x1 cones' values that extract_factors needs, and
// whatever the caller asked for in host arrays, each as one contiguous download of the vector the device formed.
//
// Exactness.  Every kernel here is compiled with contraction off, as the host code is (-ffp-contract=off), and every sum runs
// in the host loop's order, so each output equals the host path's bit for bit:
//   dual cone   one thread per column: acc from 0 over the column's entries in storage order, then base + acc, then / 2.0
//   slack       one thread per row, over the row's entries in ascending solver-order column (the order the host's column
//               scatter adds them in; prepare()'s counting sort keeps a column's duplicates in storage order), then - b / - h
// Neither kernel changes form at any length: a long column or row is one thread's longer loop, so there is no length at which
// the order of the sum could change.  The chain of additions is serial by definition of the result; the exit runs once per solve.
// The reductions are minima and maxima (order-free); the sum of squares of a second-order cone is one thread's, in order.
#pragma once
#include "solver.hip.hpp"

namespace proxsdp {
namespace dev {

#pragma clang fp contract(off)
// dc[k] = (base ? base[k] : 0) + sum_q val[q] y[row[q]], q over column k in storage order; halved where offdiag[k]
// (fix_diag_scaling(dual_cone, cones, 2.0)).  val: the caller's unscaled values.  base: c, or c + A'y of a dense A.
__global__ void __launch_bounds__(TPB)
k_exit_dual_cone(const int* __restrict__ colptr, const int* __restrict__ row, const double* __restrict__ val,
                 const double* __restrict__ y, const double* __restrict__ base, const unsigned char* __restrict__ offdiag,
                 double* __restrict__ dc, long long n) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long k = (long long)blockIdx.x * TPB + threadIdx.x; k < n; k += stride) {
        double acc = 0.0;
        for (int q = colptr[k]; q < colptr[k + 1]; ++q) acc += val[q] * y[row[q]];
        double v = (base ? base[k] : 0.0) + acc;
        if (offdiag[k]) v = v / 2.0;
        dc[k] = v;
    }
}

// slack[r] = (slack[r] + sum_q val[q] x[col[q]]) - bh[r], q over row r of the CSR (ascending column).  slack comes in as 0, or
// as A x of a dense A on the equality rows.  val: the caller's unscaled values in CSR order.
__global__ void __launch_bounds__(TPB)
k_exit_slack(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
             const double* __restrict__ x, const double* __restrict__ bh, double* __restrict__ slack, long long Q) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long r = (long long)blockIdx.x * TPB + threadIdx.x; r < Q; r += stride) {
        double acc = slack[r];
        for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) acc += val[q] * x[col[q]];
        slack[r] = acc - bh[r];
    }
}

// out[i] = v[inv[i]]: a solver-order vector into the caller's order
__global__ void __launch_bounds__(TPB)
k_exit_scatter(const double* __restrict__ v, const long long* __restrict__ inv, double* __restrict__ out, long long n) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) out[i] = v[inv[i]];
}

// out[i] = -v[i]: the block the lambda_min run reads (-lambda_max(-smat(dc)))
__global__ void __launch_bounds__(TPB)
k_exit_negate(const double* __restrict__ v, double* __restrict__ out, long long n) {
    const long long stride = (long long)gridDim.x * TPB;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) out[i] = -v[i];
}

// out[i] = v[off[i]] (the 1x1 cones' entries of the iterate)
__global__ void __launch_bounds__(TPB)
k_exit_gather(const double* __restrict__ v, const long long* __restrict__ off, int cnt, double* __restrict__ out) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < cnt) out[i] = v[off[i]];
}

// flag |= 1 when some v[i] is not finite
__global__ void __launch_bounds__(TPB)
k_exit_nonfinite(const double* __restrict__ v, long long n, int* __restrict__ flag) {
    const long long stride = (long long)gridDim.x * TPB;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) bad = bad || !isfinite(v[i]);
    if (bad) atomicOr(flag, 1);
}

// The non-PSD part of dual_feas / cone_feas (pdhg.jl:678-732), workgroup b's share into part[q * gridDim.x + b]:
//   q = 0  min y_in            q = 1  min dc over the 1x1 cones
//   q = 2  min over the second-order cones of dc[0] - sqrt(sum_{i >= 1} dc[i]^2), the sum in index order (one thread per cone)
//   q = 3  max |dc| over the variables outside every cone (k >= conelen)
// a minimum over nothing is +inf, the maximum starts at 0.  k_exit_feas_fin folds the workgroups' shares into out[0..4).
__global__ void __launch_bounds__(TPB)
k_exit_feas(const double* __restrict__ yin, long long m, const double* __restrict__ dc,
            const long long* __restrict__ one_off, int none, const long long* __restrict__ soc_off,
            const int* __restrict__ soc_len, int nsoc, long long conelen, long long n, double* __restrict__ part) {
    __shared__ double sh[4][TPB];
    const long long stride = (long long)gridDim.x * TPB;
    const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x;
    double a0 = INFINITY, a1 = INFINITY, a2 = INFINITY, a3 = 0.0;
    for (long long i = t0; i < m; i += stride) { const double v = yin[i]; a0 = v < a0 ? v : a0; }
    for (long long i = t0; i < none; i += stride) { const double v = dc[one_off[i]]; a1 = v < a1 ? v : a1; }
    for (long long i = t0; i < nsoc; i += stride) {
        const double* d = dc + soc_off[i];
        double ss = 0.0;
        for (int j = 1; j < soc_len[i]; ++j) ss += d[j] * d[j];
        const double v = d[0] - sqrt(ss);
        a2 = v < a2 ? v : a2;
    }
    for (long long k = conelen + t0; k < n; k += stride) { const double v = fabs(dc[k]); a3 = a3 < v ? v : a3; }
    sh[0][threadIdx.x] = a0; sh[1][threadIdx.x] = a1; sh[2][threadIdx.x] = a2; sh[3][threadIdx.x] = a3;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            for (int q = 0; q < 3; ++q) { const double v = sh[q][threadIdx.x + s]; if (v < sh[q][threadIdx.x]) sh[q][threadIdx.x] = v; }
            const double v = sh[3][threadIdx.x + s];
            if (sh[3][threadIdx.x] < v) sh[3][threadIdx.x] = v;
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = sh[threadIdx.x][0];
}
__global__ void __launch_bounds__(WAVE)
k_exit_feas_fin(const double* __restrict__ part, int nwg, double* __restrict__ out) {
    const int q = threadIdx.x;
    if (q >= 4) return;
    double a = part[(size_t)q * nwg];
    for (int b = 1; b < nwg; ++b) {
        const double v = part[(size_t)q * nwg + b];
        if (q < 3 ? v < a : a < v) a = v;
    }
    out[q] = a;
}
#pragma clang fp contract(fast)

}  // namespace dev

// The finite check of data the caller holds on the device, before anything is written: one reduction per array src[q] of len[q]
// doubles (null or empty: skipped) into flag[q] (cnt ints at least), read back together.  Returns the first bad array, or -1
inline int first_nonfinite_device(hipStream_t st, DevBuf<int>& flag, int cnt, const double* const* src, const int64_t* len) {
    flag.zero(st);
    for (int q = 0; q < cnt; ++q)
        if (src[q] && len[q] > 0)
            hipLaunchKernelGGL(dev::k_exit_nonfinite, dim3(grid_for(len[q])), dim3(dev::TPB), 0, st, src[q], (long long)len[q], flag.p + q);
    PX_HIP(hipGetLastError());
    std::vector<int> h((size_t)cnt, 0);
    flag.download(h.data(), (size_t)cnt, st);
    PX_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < cnt; ++q)
        if (h[q]) return q;
    return -1;
}
// throws by the first bad array's name
inline void require_finite_device(hipStream_t st, DevBuf<int>& flag, int cnt, const double* const* src, const int64_t* len,
                                  const char* const* name, const char* what) {
    const int q = first_nonfinite_device(st, flag, cnt, src, len);
    if (q >= 0) throw std::invalid_argument(std::string(what) + ": non-finite entry in " + name[q]);
}
// one array, the whole message the caller's
inline void require_finite_device(hipStream_t st, DevBuf<int>& flag, const double* v, int64_t len, const std::string& message) {
    if (first_nonfinite_device(st, flag, 1, &v, &len) >= 0) throw std::invalid_argument(message);
}

// the in-place quirks of cache_solution (pdhg.jl:749-755): fix_diag_scaling on pair.x, then x = D x, y = E y
inline void Solver::exit_rescale_iterate() {
    const double inv = 1.0 / std::sqrt(2.0);
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
        const BlockInfo& B = P.blocks[idx];
        if (B.n < 2) continue;
        const int nt = ceil_div(B.n, dev::TILE);
        hipLaunchKernelGGL(dev::k_scale_offdiag, dim3(nt * (nt + 1) / 2), dim3(dev::TPB), 0, stream,
                           xbuf[xc].p + B.off, B.n, inv);
    }
    if (P.equilibrated) {                                    // pair.x = D*pair.x; pair.y = E*pair.y (pdhg.jl:751-755)
        if (Ddiag_d.n == 0) {
            Ddiag_d.alloc(P.n); Ediag_d.alloc(std::max<int64_t>(P.Q, 1));
            Ddiag_d.upload(P.Ddiag.data(), P.n, stream); Ediag_d.upload(P.Ediag.data(), P.Q, stream);
        }
        hipLaunchKernelGGL(dev::k_scale_by, dim3(grid_for(P.n)), dim3(dev::TPB), 0, stream, xbuf[xc].p, Ddiag_d.p, (long long)P.n);
        hipLaunchKernelGGL(dev::k_scale_by, dim3(grid_for(std::max<int64_t>(P.Q, 1))), dim3(dev::TPB), 0, stream,
                           rs.ybuf[yc].p, Ediag_d.p, (long long)P.Q);
    }
}

// workgroups of the feasibility reductions: the longest of the free tail, m inequality rows, the 1x1 cones and the SOCs
inline int Solver::exit_feas_grid(int64_t m) const {
    size_t ones = 0;
    for (const BlockInfo& B : P.blocks) ones += B.n == 1 ? 1 : 0;
    return grid_for(std::max<int64_t>(std::max(P.n - P.conelen, m), (int64_t)std::max(ones, P.socs.size())));
}

// what the exit kernels read beside the operator's pattern (csc_ptr / csc_row, csr_ptr / csr_col: upload_sparse_operator):
// uploaded once, at the first exit; the row-sized part is the row state's (RowState::build_exit)
inline void Solver::exit_device_setup() {
    if (xd.ready) return;
    const size_t nz = (size_t)std::max<int64_t>(P.nnz, 1), n1 = (size_t)std::max<int64_t>(P.n, 1);
    rs.build_exit(P.p, P.m, P.nnz, exit_feas_grid(P.m));
    std::vector<double> rv(nz, 0.0);                         // the unscaled values in CSR order: prepare()'s counting sort again
    {
        std::vector<int64_t> cur(P.rowptr.begin(), P.rowptr.end() - 1);
        for (int64_t k = 0; k < P.n; ++k)
            for (int64_t q = P.colptr[k]; q < P.colptr[k + 1]; ++q) rv[cur[P.rowidx[q]]++] = P.val_orig[q];
    }
    rs.exit.cval.upload(P.val_orig.data(), P.nnz, stream);
    rs.exit.rval.upload(rv.data(), P.nnz, stream);
    xd.c.alloc(n1); xd.c.upload(P.c_orig.data(), P.n, stream);
    const std::vector<double> bh = stacked_bh(P.b_orig, P.h_orig);
    rs.exit.bh.upload(bh.data(), P.Q, stream);
    static_assert(sizeof(long long) == sizeof(int64_t), "the inverse order is uploaded as it is");
    xd.inv.alloc(n1); xd.inv.upload(reinterpret_cast<const long long*>(P.inv.data()), P.n, stream);
    if (offdiag_d.n == 0) { offdiag_d.alloc(n1); offdiag_d.upload(P.offdiag.data(), P.n, stream); }
    std::vector<long long> ones, so;
    std::vector<int> sl;
    for (size_t idx = 0; idx < P.blocks.size(); ++idx)
        if (P.blocks[idx].n == 1) { xd.ones.push_back((int)idx); ones.push_back(P.blocks[idx].off); }
    for (const SocInfo& S : P.socs) { so.push_back(S.off); sl.push_back(S.len); }
    xd.one_off.alloc(std::max<size_t>(ones.size(), 1)); xd.one_off.upload(ones.data(), ones.size(), stream);
    xd.soc_off.alloc(std::max<size_t>(so.size(), 1)); xd.soc_off.upload(so.data(), so.size(), stream);
    xd.soc_len.alloc(std::max<size_t>(sl.size(), 1)); xd.soc_len.upload(sl.data(), sl.size(), stream);
    xd.dc.alloc(n1);
    if (P.dense()) { xd.base.alloc(n1); xd.zero.alloc(n1); xd.zero.zero(stream); }
    xd.scal.alloc(4);
    PX_HIP(hipStreamSynchronize(stream));                    // (the host vectors above go out of scope)
    xd.ready = true;
}

// M x - [b; h] into rs.exit.slack and the dual cone c + M'y (halved off the diagonals) into xd.dc, from the rescaled iterate
inline void Solver::exit_form_vectors(bool zero_c) {
    const double* x = xbuf[xc].p;
    const double* y = rs.ybuf[yc].p;
    if (P.Q > 0) {
        rs.exit.slack.zero(stream);
        if (P.dense() && P.p > 0) dense_mv(x, rs.exit.slack.p, false);        // A x with the caller's (unscaled) dense A
        hipLaunchKernelGGL(dev::k_exit_slack, dim3(grid_for(P.Q)), dim3(dev::TPB), 0, stream,
                           (const int*)rs.csr_ptr.p, (const int*)rs.csr_col.p, (const double*)rs.exit.rval.p, x, (const double*)rs.exit.bh.p,
                           rs.exit.slack.p, (long long)P.Q);
    }
    if (P.n > 0) {
        const double* base = zero_c ? nullptr : xd.c.p;
        if (P.dense()) {                                                 // c + A'y with the caller's (unscaled) dense A
            dense_mtv(1, y, 0, false, xd.base.p, 0, nullptr, zero_c ? xd.zero.p : xd.c.p, nullptr, 0, false);
            base = xd.base.p;
        }
        hipLaunchKernelGGL(dev::k_exit_dual_cone, dim3(grid_for(P.n)), dim3(dev::TPB), 0, stream,
                           (const int*)rs.csc_ptr.p, (const int*)rs.csc_row.p, (const double*)rs.exit.cval.p, y, base,
                           (const unsigned char*)offdiag_d.p, xd.dc.p, (long long)P.n);
    }
    PX_HIP(hipGetLastError());
}

// the four violations that need no eigenvalue, from xd.dc and the rescaled y: inequality duals, 1x1 cones, second-order
// cones, free variables -- the host path's expressions on the extrema the device reduced
inline void Solver::exit_cone_violations(double viol[4]) {
    hipLaunchKernelGGL(dev::k_exit_feas, dim3(rs.exit.feas_wg), dim3(dev::TPB), 0, stream,
                       (const double*)rs.ybuf[yc].p + P.p, (long long)P.m, (const double*)xd.dc.p,
                       (const long long*)xd.one_off.p, (int)xd.ones.size(), (const long long*)xd.soc_off.p,
                       (const int*)xd.soc_len.p, (int)P.socs.size(), (long long)P.conelen, (long long)P.n, rs.exit.part.p);
    hipLaunchKernelGGL(dev::k_exit_feas_fin, dim3(1), dim3(dev::WAVE), 0, stream, (const double*)rs.exit.part.p, rs.exit.feas_wg, xd.scal.p);
    PX_HIP(hipGetLastError());
    double ext[4];
    xd.scal.download(ext, 4, stream);
    PX_HIP(hipStreamSynchronize(stream));
    viol[0] = P.m > 0 ? -std::min(0.0, ext[0]) : 0.0;
    viol[1] = std::max(0.0, -std::min(0.0, ext[1]));
    viol[2] = std::max(0.0, -std::min(0.0, ext[2]));
    viol[3] = ext[3];
}

// the six vectors in the caller's order and units: into the caller's device buffers (dv, may be NULL) and / or host arrays.
// primal and dual_cone are scattered on the device (into the caller's buffer when there is one); duals and slacks are
// contiguous copies.  Returns with every write complete.
inline void Solver::exit_write_vectors(const proxsdp_device_vectors* dv, double* primal, double* dual_cone, double* dual_eq,
                                       double* dual_in, double* slack_eq, double* slack_in) {
    auto scattered = [&](const double* v, double* devout, double* host, DevBuf<double>& own) {
        if ((!devout && !host) || P.n == 0) return;
        double* dst = devout;
        if (!dst) { if (own.n == 0) own.alloc(P.n); dst = own.p; }
        hipLaunchKernelGGL(dev::k_exit_scatter, dim3(grid_for(P.n)), dim3(dev::TPB), 0, stream, v, (const long long*)xd.inv.p,
                           dst, (long long)P.n);
        if (host) PX_HIP(hipMemcpyAsync(host, dst, (size_t)P.n * sizeof(double), hipMemcpyDeviceToHost, stream));
    };
    auto copied = [&](const double* v, int64_t len, double* devout, double* host) {
        if (len == 0) return;
        if (devout) PX_HIP(hipMemcpyAsync(devout, v, (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, stream));
        if (host) PX_HIP(hipMemcpyAsync(host, v, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, stream));
    };
    scattered(xbuf[xc].p, dv ? dv->primal : nullptr, primal, xd.prim);
    scattered(xd.dc.p, dv ? dv->dual_cone : nullptr, dual_cone, xd.dcone);
    copied(rs.ybuf[yc].p, P.p, dv ? dv->dual_eq : nullptr, dual_eq);
    copied(rs.ybuf[yc].p + P.p, P.m, dv ? dv->dual_in : nullptr, dual_in);
    copied(rs.exit.slack.p, P.p, dv ? dv->slack_eq : nullptr, slack_eq);
    copied(rs.exit.slack.p + P.p, P.m, dv ? dv->slack_in : nullptr, slack_in);
    PX_HIP(hipGetLastError());
    PX_HIP(hipStreamSynchronize(stream));
}

// cache_solution on the device.  zero_c: the certificate snapshot that zeroes c (finish(), stop_reason == 6).
inline void Solver::cache_solution_device(bool zero_c) {
    double t0 = now_s();
    exit_rescale_iterate();
    exit_device_setup();
    exit_form_vectors(zero_c);
    // the factors of this snapshot's PSD blocks, before the lambda_min Lanczos below reuses the blocks' workspaces
    if (req.factors_out) {
        std::vector<double> one_vals(P.blocks.size(), 0.0);
        if (!xd.ones.empty()) {
            const int cnt = (int)xd.ones.size();
            std::vector<double> h(cnt);
            xd.onev.alloc(cnt);
            hipLaunchKernelGGL(dev::k_exit_gather, dim3(ceil_div(cnt, dev::TPB)), dim3(dev::TPB), 0, stream,
                               (const double*)xbuf[xc].p, (const long long*)xd.one_off.p, cnt, xd.onev.p);
            xd.onev.download(h.data(), cnt, stream);
            PX_HIP(hipStreamSynchronize(stream));
            for (int i = 0; i < cnt; ++i) one_vals[xd.ones[i]] = h[i];
        }
        extract_factors(one_vals);
    }
    double viol[4];
    exit_cone_violations(viol);
    double sdp_viol = std::max(viol[1], viol[2]);
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
        const BlockInfo& B = P.blocks[idx];
        if (B.n == 1) continue;
        const double* blk = xd.dc.p + B.off;
        const double mn = dual_block_min_eig(idx, [&](double* tmp, bool negated) {
            if (negated)
                hipLaunchKernelGGL(dev::k_exit_negate, dim3(grid_for(B.N)), dim3(dev::TPB), 0, stream, blk, tmp, (long long)B.N);
            else
                PX_HIP(hipMemcpyAsync(tmp, blk, (size_t)B.N * sizeof(double), hipMemcpyDeviceToDevice, stream));
        });
        sdp_viol = std::max(sdp_viol, -std::min(0.0, mn));
    }
    const double dfeas = std::max({sdp_viol, viol[0], viol[3]});
    exit_write_vectors(req.out_dev, res.primal, res.dual_cone, res.dual_eq, res.dual_in, res.slack_eq, res.slack_in);
    finish_snapshot(dfeas);
    st.exit_time += now_s() - t0;
}

// proxsdp_hip_solve_device: the finite check of the start vectors the caller holds on the device (the host entry checks
// every host array before the device exists; this one check needs it)
inline void Solver::check_start_dev() {
    const proxsdp_device_vectors& d = *req.start_dev;
    const double* v[3] = {d.primal, d.dual_eq, d.dual_in};
    const int64_t len[3] = {P.n, P.p, P.m};
    const char* name[3] = {"primal", "dual_eq", "dual_in"};
    DevBuf<int> flag(3);
    require_finite_device(stream, flag, 3, v, len, name, "proxsdp_device_vectors (start)");
}

// proxsdp_hip_exit_vectors: the exit path's own launches on a host iterate (include/proxsdp_hip.h)
inline void Solver::test_exit_vectors(const double* x, const double* y, bool zero_c, double* primal, double* dual_cone,
                                      double* dual_eq, double* dual_in, double* slack_eq, double* slack_in, double* viol,
                                      double* neg, int64_t neg_cap) {
    int64_t need = 0;
    for (const BlockInfo& B : P.blocks) if (B.n >= 2) need += B.N;
    if (neg_cap < need || (need > 0 && !neg)) throw std::invalid_argument("exit vectors: neg_cap is smaller than the PSD blocks of side >= 2");
    setup_device();
    setup_dense_scaling();
    alloc_iterate_pairs();
    upload_sparse_operator();
    if (P.dense()) upload_dense();
    xbuf[xc].upload(x, P.n, stream);
    rs.ybuf[yc].upload(y, P.Q, stream);
    exit_rescale_iterate();
    exit_device_setup();
    exit_form_vectors(zero_c);
    double v4[4];
    exit_cone_violations(v4);
    if (viol) std::copy(v4, v4 + 4, viol);
    DevBuf<double> tmp((size_t)std::max<int64_t>(need, 1));
    int64_t at = 0;
    for (const BlockInfo& B : P.blocks) {
        if (B.n < 2) continue;
        hipLaunchKernelGGL(dev::k_exit_negate, dim3(grid_for(B.N)), dim3(dev::TPB), 0, stream, (const double*)xd.dc.p + B.off,
                           tmp.p + at, (long long)B.N);
        at += B.N;
    }
    PX_HIP(hipGetLastError());
    tmp.download(neg, need, stream);
    exit_write_vectors(nullptr, primal, dual_cone, dual_eq, dual_in, slack_eq, slack_in);
}

}  // namespace proxsdp
