// Hooks of the kernel-level test entry points (capi.hip): each one puts host data where a solve would have it, runs the
// solver's own launch code on it and copies the outputs back.
#pragma once
#include "solver.hip.hpp"
#include "lanczos.hip.hpp"

namespace proxsdp {

// d <- `count` copies of the sentinel
static inline void filled(DevBuf<double>& d, size_t count, double sentinel, hipStream_t s) {
    std::vector<double> h(count, sentinel);
    d.alloc(count);
    d.upload(h.data(), count, s);
    PX_HIP(hipStreamSynchronize(s));
}

inline void Solver::test_project(int idx, double* xp, int tr) {
    target_rank.assign(1, tr); current_rank.assign(1, 0); min_eig.assign(1, 0.0);
    iter = 1;
    project_block(idx, xp - P.blocks[idx].off, xp - P.blocks[idx].off, false);
}
// the iterate's buffers as the "Init" section allocates them (x, M'y: n; y, Mx: Q; two of each), zeroed
inline void Solver::test_spmv(bool transpose, const double* in, double* out) {
    setup_device();
    upload_sparse_operator();
    if (transpose) {
        // M'y as the linesearch computes it: ONE plain candidate against a zero M'y_old
        alloc_iterate_pairs();
        use_support = false;
        alloc_candidates();
        rs.ycand_d.upload(in, P.Q, stream);
        dev::TrialBatch tb{};
        tb.nc = 1; tb.plain = 1;
        batch_mty(tb, 1);
        Mtycand_d.download(out, P.n, stream);
    } else {
        DevBuf<double> xin(std::max<int64_t>(P.n, 1)), xout(std::max<int64_t>(P.Q, 1));
        xin.upload(in, P.n, stream);
        spmv(xin.p, xout.p);
        xout.download(out, P.Q, stream);
    }
    PX_HIP(hipStreamSynchronize(stream));
}
// one batch of the linesearch on host data (include/proxsdp_hip.h proxsdp_trial_batch).  The problem was prepared with every
// row of M as an equality row (no cones: columns keep their order and their storage order); p is set here.
inline void Solver::test_trial_batch(proxsdp_trial_batch& t) {
    const int64_t n = P.n, Q = P.Q;
    if (n < 1 || Q < 1 || t.p < 0 || t.p > Q || t.nc < 1 || t.nc > NCAND || t.c0 >= t.nc)
        throw std::invalid_argument("trial batch: n, Q >= 1, 0 <= p <= Q, 1 <= nc <= 3, c0 < nc");
    if (t.support < 0 || t.support > 2) throw std::invalid_argument("trial batch: support must be 0, 1 or 2");
    if (!t.bh || !t.y || !t.Mx || !t.Mx_old || !t.x || !t.x_old || !t.Mty_old || !t.y_out || !t.Mty_out || !t.scal ||
        (t.c0 >= 0 && !t.scal_re) || (t.support == 1 && (!t.supp_out || !t.x_upd || !t.xsave || !t.esv)))
        throw std::invalid_argument("trial batch: NULL array");
    P.p = t.p; P.m = Q - t.p;
    setup_device();
    upload_sparse_operator();
    alloc_iterate_pairs();
    c_d.alloc(n); c_d.upload(P.c.data(), n, stream);
    rs.bh_d.upload(t.bh, Q, stream);
    if (t.roww) { roww_d.alloc(Q); roww_d.upload(t.roww, Q, stream); }
    rs.ybuf[yc].upload(t.y, Q, stream);
    rs.Mxbuf[1 - mxc].upload(t.Mx, Q, stream); rs.Mxbuf[mxc].upload(t.Mx_old, Q, stream);
    xbuf[xc].upload(t.x_old, n, stream);
    PX_HIP(hipStreamSynchronize(stream));
    use_support = t.support == 1;
    general_row_weights = t.support == 2;                // (the general path of a block-sharded solve: weighted b'y, h'y)
    if (use_support) {
        const std::vector<int> supp = support_list();
        upload_support(supp);
        n_res_wg = 0; rstride = 0;                       // (no reconstruction ran: no off-support partials)
        respart_d.alloc(2); respart_d.zero(stream);
        std::vector<double> mtyS(std::max(ns, 1), 0.0);
        for (int s = 0; s < ns; ++s) mtyS[s] = t.Mty_old[supp[s]];
        MtyS_cur.upload(mtyS.data(), ns, stream);
        // primal_step!'s update on the support, in place on x_old; the new iterate (what the projection would write) is t.x
        launch_primal_update_S(xbuf[xc].p, t.tau_update);
        xbuf[xc].download(t.x_upd, n, stream);
        xsave_d.download(t.xsave, ns, stream);
        esv_d.download(t.esv, (size_t)2 * ns, stream);
        std::copy(supp.begin(), supp.end(), t.supp_out);
        PX_HIP(hipStreamSynchronize(stream));
    } else {
        Mtybuf[mtyc].upload(t.Mty_old, n, stream);
    }
    t.ns = batch_shape().cnt;
    xbuf[1 - xc].upload(t.x, n, stream);
    alloc_candidates();
    dev::TrialBatch tb{};
    tb.nc = t.nc; tb.plain = t.plain;
    for (int c = 0; c < t.nc; ++c) { tb.tau[c] = t.tau[c]; tb.theta[c] = t.theta[c]; tb.bt[c] = t.bt[c]; tb.sigma[c] = t.sigma[c]; }
    batch_evaluate(tb, t.nc, t.xold_coef);
    const double* rec = batch_read_back(t.nc);
    std::copy(rec, rec + (size_t)t.nc * NSCAL, t.scal);
    const BatchShape b = batch_shape();
    t.gq = b.gq; t.gx = b.gx;
    for (int c = 0; c < t.nc; ++c) {
        PX_HIP(hipMemcpyAsync(t.y_out + (size_t)c * Q, rs.ycand_d.p + (size_t)c * b.ystride, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (t.ns > 0)
            PX_HIP(hipMemcpyAsync(t.Mty_out + (size_t)c * t.ns, Mtycand_d.p + (size_t)c * b.mstride, (size_t)t.ns * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    PX_HIP(hipStreamSynchronize(stream));
    if (t.c0 >= 0) {                                     // the re-evaluation leg: candidate c0's residuals with the final steps
        dev::TrialBatch t1{};
        t1.nc = 1; t1.tau[0] = t.tau_re; t1.theta[0] = t.theta[t.c0]; t1.bt[0] = t.sigma_re; t1.sigma[0] = t.sigma_re;
        batch_residuals(t1, 1, t.c0, t.xold_coef);
        rec = batch_read_back(1);
        std::copy(rec, rec + NSCAL, t.scal_re);
    }
}
// the cone tail on host data: SOC gap, SOC projection, SOC gap again, then the 1x1 PSD blocks (disjoint entries)
inline void Solver::test_cone_tail(const double* x, int64_t n, const int64_t* so, const int32_t* sl, int nsoc,
                                   const int64_t* oo, int none, double* x_soc, double* gap_in, double* gap_out,
                                   double* x_clamp, double* mineig) {
    DevBuf<double> xd(std::max<int64_t>(n, 1));
    xd.upload(x, n, stream);
    if (nsoc > 0) {
        std::vector<long long> off(so, so + nsoc);
        std::vector<int> len(sl, sl + nsoc);
        soc_off.alloc(nsoc); soc_len.alloc(nsoc); soc_gap_d.alloc(nsoc);
        soc_off.upload(off.data(), nsoc, stream); soc_len.upload(len.data(), nsoc, stream);
        launch_soc_gap(xd.p, nsoc);
        soc_gap_d.download(gap_in, nsoc, stream);
        launch_soc_project(xd.p, nsoc);
        launch_soc_gap(xd.p, nsoc);
        soc_gap_d.download(gap_out, nsoc, stream);
        PX_HIP(hipStreamSynchronize(stream));            // host vectors go out of scope
    }
    xd.download(x_soc, n, stream);
    if (none > 0) {
        std::vector<long long> off(oo, oo + none);
        one_off.alloc(none); one_min.alloc(none);
        one_off.upload(off.data(), none, stream);
        launch_clamp_scalars(xd.p, none);
        one_min.download(mineig, none, stream);
        PX_HIP(hipStreamSynchronize(stream));
    }
    xd.download(x_clamp, n, stream);
    PX_HIP(hipStreamSynchronize(stream));
}

// one PSD projection of host data through the phases of setup() that the projection needs and psd_projection itself: the
// block lists, the small-block batch with its rank record, the 1x1 offsets -- no launch of its own
inline void Solver::test_project_cones(proxsdp_project_cones& t) {
    if (P.n < 1) throw std::invalid_argument("project cones: the problem has no variables");
    if (!t.x || !t.x_out || (!P.blocks.empty() && (!t.block_off || !t.block_side || !t.block_class || !t.rank || !t.min_eig || !t.sweeps)))
        throw std::invalid_argument("project cones: NULL array");
    init_parameters();
    setup_device();
    classify_blocks();
    setup_small_batch();
    setup_soc();
    DevBuf<double> xd(P.n);
    xd.upload(t.x, P.n, stream);
    iter = 1;
    psd_projection(xd.p);
    xd.download(t.x_out, P.n, stream);
    std::vector<double> ones(one_blocks.size());
    if (!one_blocks.empty()) one_min.download(ones.data(), ones.size(), stream);
    PX_HIP(hipStreamSynchronize(stream));
    harvest_small_ranks();
    merge_block_stats();
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
        t.block_off[idx] = P.blocks[idx].off; t.block_side[idx] = P.blocks[idx].n;
        t.block_class[idx] = P.blocks[idx].n == 1 ? 0 : 3;
        t.rank[idx] = current_rank[idx]; t.min_eig[idx] = min_eig[idx]; t.sweeps[idx] = -1;
    }
    for (size_t q = 0; q < one_blocks.size(); ++q) t.min_eig[one_blocks[q]] = ones[q];
    for (size_t q = 0; q < small_blocks.size(); ++q) {
        const int idx = small_blocks[q];
        t.block_class[idx] = P.blocks[idx].n <= small_jacobi_max ? 1 : 2;
        if (q < small_sweeps.size()) t.sweeps[idx] = small_sweeps[q];
    }
    t.batched_small_eigs = st.batched_small_eigs; t.full_eigs = st.full_eigs; t.full_eigs_sign = st.full_eigs_sign;
    t.sign_short_pass = st.sign_short_pass; t.sign_short_fail = st.sign_short_fail;
}

// ONE product of the sign iteration on host data (include/proxsdp_hip.h proxsdp_sym_product), launched by sym_gemm itself on the
// tile shape asked for.  eig[0] was sized for side t.n (alloc_eigwork); operands are zero-padded to ld as full_eig_by_sign
// leaves its work matrices, every output buffer is prefilled with the sentinel.
inline void Solver::test_sym_product(proxsdp_sym_product& t) {
    EigWork& W = eig[0];
    const int n = W.n, ld = W.nt * dev::TILE;
    const int64_t N = W.N;
    const bool fin = t.epilogue >= 2, fuse = t.epilogue == 3;
    if (t.tile != 32 && t.tile != 48 && t.tile != 64) throw std::invalid_argument("sym product: tile must be 32, 48 or 64");
    if (t.epilogue < 0 || t.epilogue > 3) throw std::invalid_argument("sym product: epilogue must be 0 .. 3");
    if (fin && t.tile != 64) throw std::invalid_argument("sym product: the final product runs on 64 x 64 tiles only");
    if (t.tile == 48 && !sign_tile48_fits(n, ld))
        throw std::invalid_argument("sym product: 48 x 48 tiles do not fit this side (48 ceil(n / 48) > ld, or no LDS grant)");
    if (!t.P || !t.Q || (t.epilogue == 1 && !t.Y) || (!fin && !t.T) || (fin && (!t.xp || !t.part)) ||
        (fuse && (!t.xold || !t.mask || !t.respart || t.mask_off < 0 || t.mask_words * 32 < t.mask_off + N)))
        throw std::invalid_argument("sym product: missing buffer");
    W.sg_ld = ld;
    W.sg_small = t.tile != 64;
    W.sg_nt48 = t.tile == 48 ? ceil_div(n, dev::SG_T48) : 0;
    const int grid = sym_gemm_grid(W, fin);
    const size_t sz = (size_t)ld * ld;
    std::vector<double> pad(sz);
    auto padded = [&](const double* M, DevBuf<double>& d) {
        std::fill(pad.begin(), pad.end(), 0.0);
        for (int j = 0; j < n; ++j) std::copy(M + (size_t)j * n, M + (size_t)j * n + n, pad.begin() + (size_t)j * ld);
        d.alloc(sz);
        d.upload(pad.data(), sz, stream);
        PX_HIP(hipStreamSynchronize(stream));
    };
    DevBuf<double> dP, dQ, dY, dT, dpart, dsc, dxp, dxold;
    padded(t.P, dP); padded(t.Q, dQ);
    if (t.epilogue == 1) padded(t.Y, dY);
    if (!fin) filled(dT, sz, t.sentinel, stream);
    if (t.part) filled(dpart, grid, t.sentinel, stream);
    if (t.use_dsc) { dsc.alloc(3); dsc.upload(t.dsc, 3, stream); }
    if (fin) filled(dxp, N, t.sentinel, stream);
    if (fuse) {
        dxold.alloc(N); dxold.upload(t.xold, N, stream);
        mask_d.alloc(t.mask_words); mask_d.upload(t.mask, t.mask_words, stream);
        P.blocks.assign(1, BlockInfo{n, N, t.mask_off});
        tile_base.assign(1, 0);
        rstride = grid;
        filled(respart_d, (size_t)2 * grid, t.sentinel, stream);
    }
    const double* sc = t.use_dsc ? dsc.p : nullptr;
    switch (t.epilogue) {
        case 0: sym_gemm<dev::SG_PLAIN, false>(W, dP.p, dQ.p, dT.p, nullptr, t.ca, t.cb, t.cc, sc, dpart.p, nullptr, nullptr, -1); break;
        case 1: sym_gemm<dev::SG_POLY, false>(W, dP.p, dQ.p, dT.p, dY.p, t.ca, t.cb, t.cc, sc, dpart.p, nullptr, nullptr, -1); break;
        case 2: sym_gemm<dev::SG_FINAL, false>(W, dP.p, dQ.p, nullptr, nullptr, t.ca, t.cb, t.cc, sc, dpart.p, dxp.p, nullptr, -1); break;
        default: sym_gemm<dev::SG_FINAL, true>(W, dP.p, dQ.p, nullptr, nullptr, t.ca, t.cb, t.cc, sc, dpart.p, dxp.p, dxold.p, 0); break;
    }
    PX_HIP(hipGetLastError());
    if (!fin) dT.download(t.T, sz, stream);
    if (t.part) dpart.download(t.part, grid, stream);
    if (fin) dxp.download(t.xp, N, stream);
    if (fuse) respart_d.download(t.respart, (size_t)2 * grid, stream);
    PX_HIP(hipStreamSynchronize(stream));
    t.ld = ld;
    t.grid = grid;
}

// The head of a sign projection on a packed block (eig[0] sized for it): k_unpack_sym into a matrix prefilled with the sentinel
// (A, ld x ld: what the kernel writes and what it leaves), then -- on a cleared matrix, the tile shape the solver chooses --
// sign_unpack and sign_scale as full_eig_by_sign runs them; sc[16] as k_sign_scalars documents it.
inline void Solver::test_sign_unpack(const double* packed, double sentinel, double* A, double* sc) {
    EigWork& W = eig[0];
    const int ld = W.nt * dev::TILE;
    const size_t sz = (size_t)ld * ld;
    DevBuf<double> xp(W.N), As(sz), dsc(16);
    xp.upload(packed, W.N, stream);
    std::vector<double> h(sz, sentinel);
    As.upload(h.data(), sz, stream);
    W.sgA.alloc(sz); W.sgY.alloc(sz);
    W.sgA.zero(stream); W.sgY.zero(stream);
    W.sg_ld = ld;
    sign_choose_tiles(W);
    W.sg_part.alloc(W.sg_npart);
    dsc.zero(stream);
    sign_unpack(W, xp.p, As.p, dsc.p);
    sign_unpack(W, xp.p, W.sgA.p, dsc.p);
    sign_scale(W, dsc.p);
    PX_HIP(hipGetLastError());
    As.download(A, sz, stream);
    dsc.download(sc, 16, stream);
    PX_HIP(hipStreamSynchronize(stream));
}

// ONE rank-r reconstruction on host data (include/proxsdp_hip.h proxsdp_reconstruct_fused) through launch_reconstruct, as
// ritz_pairs_to_block calls it on the support path: eig[0] was sized for side t.n, the block sits at packed offset mask_off of
// a vector whose support mask is t.mask, its residual slots start at slot 0 of a buffer of stride grid.  xp and the whole of
// respart (respart_cap slots: whatever lies behind 2 grid is a guard zone) are prefilled with the sentinel.
inline void Solver::test_reconstruct_fused(proxsdp_reconstruct_fused& t) {
    EigWork& W = eig[0];
    const int n = W.n, r = t.r;
    const int64_t N = W.N;
    const bool fuse = t.xold != nullptr;
    const int grid = W.napart;
    if (t.respart_cap < 2 * (int64_t)grid) throw std::invalid_argument("reconstruct: respart_cap < 2 grid");
    DevBuf<double> dZ(std::max<size_t>(1, (size_t)t.ldz * r)), dlam(std::max(1, r)), dxp, dxold;
    dZ.upload(t.Z, (size_t)t.ldz * r, stream);
    dlam.upload(t.lam, r, stream);
    filled(dxp, N, t.sentinel, stream);
    filled(respart_d, (size_t)t.respart_cap, t.sentinel, stream);
    use_support = fuse;
    if (fuse) {
        dxold.alloc(N); dxold.upload(t.xold, N, stream);
        mask_d.alloc(t.mask_words); mask_d.upload(t.mask, t.mask_words, stream);
        P.blocks.assign(1, BlockInfo{n, N, t.mask_off});
        tile_base.assign(1, 0);
        rstride = grid;
    }
    const auto before = W.lst.mfma_reconstructions;
    launch_reconstruct(W, dZ.p, t.ldz, dlam.p, r, dxp.p, fuse ? dxold.p : nullptr, fuse ? 0 : -1);
    PX_HIP(hipGetLastError());
    dxp.download(t.xp, N, stream);
    respart_d.download(t.respart, (size_t)t.respart_cap, stream);
    PX_HIP(hipStreamSynchronize(stream));
    t.grid = grid;
    t.kernel = W.lst.mfma_reconstructions > before ? 1 : 0;
}

// ONE basis rotation on host data (include/proxsdp_hip.h proxsdp_rotation) through Solver::rotate -- the pinned staging copy of
// U, its upload and rotate_launch -- from W.V into W.Z, as the restart and the final Ritz-vector rotation run it.  eig[0] was
// sized for a Krylov dimension that holds every column named; V goes into the zeroed basis (padding rows stay zero, as the
// step kernels leave them), the first out_cols columns of Z are prefilled with the sentinel.
inline void Solver::test_rotate(proxsdp_rotation& t) {
    EigWork& W = eig[0];
    const int n = W.n, npad = W.npad;
    if (W.wide != (t.wide != 0)) throw std::logic_error("rotation: the workspace is not the one asked for");
    if (std::max(t.Kv, t.out_cols) > W.cap) throw std::logic_error("rotation: workspace too small");
    std::vector<double> h((size_t)npad * std::max(t.Kv, t.out_cols), 0.0);
    for (int j = 0; j < t.Kv; ++j) std::copy(t.V + (size_t)j * n, t.V + (size_t)j * n + n, h.begin() + (size_t)j * npad);
    W.V.upload(h.data(), (size_t)npad * t.Kv, stream);
    PX_HIP(hipStreamSynchronize(stream));
    std::fill(h.begin(), h.end(), t.sentinel);
    W.Z.upload(h.data(), (size_t)npad * t.out_cols, stream);
    PX_HIP(hipStreamSynchronize(stream));
    W.lzrun.plan.engine = t.wide != 0 ? LzEngine::wide : LzEngine::step;
    const std::vector<double> U(t.U, t.U + (size_t)t.K * t.ncols);
    // behind U, where a restart's arrow part rides in the same upload: NaN, which no kernel may take for rows of U
    const std::vector<double> behind(8, std::numeric_limits<double>::quiet_NaN());
    rotate(W, t.K, U, t.K, t.ncols, W.Z.p, t.copy_src, t.copy_dst, behind.data(), (int)behind.size());
    PX_HIP(hipGetLastError());
    W.Z.download(t.out, (size_t)npad * t.out_cols, stream);
    PX_HIP(hipStreamSynchronize(stream));
    t.npad = npad;
    t.form = W.rot_form;
    t.launches = W.rot_launches;
}

// Where the per-cycle observer of a captured Lanczos run writes (the arrays of proxsdp_lanczos_cycles or proxsdp_operator_cycles,
// prefilled by the capi entry), and `more`: what an entry reports on top of info[0 .. 9]
struct LzCycleSink {
    int nev, max_cycles, cols, ldv, info_ld;
    double sentinel;
    int32_t* info; double* V; double* alphas; double* betas; double* D; double* f;
    int32_t* cycles;
    std::function<void(EigWork&, LzRun&, int32_t*)> more;
    bool positive_part = false;                  // the run is lanczos(W, xp, nev, true) (proxsdp_hip_positive_part)
};

// Every cycle of ONE run of Solver::lanczos (include/proxsdp_hip.h proxsdp_lanczos_cycles, proxsdp_operator_cycles): the driver's
// observer copies out what the cycle left -- the whole basis buffer, the record's coefficients, the arrow part in R.T and what
// the plan and the restart before it decided -- and the driver itself ends the run after max_cycles (the options' maxiter).
// eig[0] was sized for the run's Krylov dimension; the capi entry prefilled the caller's arrays.
inline void Solver::test_observed_run(const LzCycleSink& t, const double* xp) {
    EigWork& W0 = eig[0];
    const int cols = t.cols, npad = W0.npad;
    const int kd = t.positive_part ? lz_positive_part_dim(W0.cap, krylov_dim(t.nev), t.nev, (int)opt.full_eig_lanczos_kdim10) : krylov_dim(t.nev);
    if (npad != t.ldv || cols > W0.cap || kd + 1 != cols) throw std::logic_error("lanczos cycles: the workspace is not the one asked for");
    int c = 0;
    DevBuf<double> again;
    std::vector<double> again_h;
    const std::function<void(EigWork&, LzRun&)> observe = [&](EigWork& W, LzRun& R) {
        if (c >= t.max_cycles) throw std::logic_error("lanczos cycles: the driver ran past max_cycles");
        if (R.krylovdim + 1 != cols) throw std::logic_error("lanczos cycles: the run's Krylov dimension is not the one asked for");
        const LzRecord rec(R.plan.rec.host, R.plan.rec.ld);
        const int kfirst = R.kfirst, Kend = rec.ctl.stop ? rec.ctl.kstop : R.krylovdim;
        if (Kend < kfirst || Kend > R.krylovdim) throw std::logic_error("lanczos cycles: kstop outside the cycle");
        int32_t* info = t.info + (size_t)t.info_ld * c;
        info[0] = kfirst; info[1] = Kend; info[2] = rec.ctl.stop;
        info[3] = R.plan.engine == LzEngine::wide ? PROXSDP_LZ_ENGINE_WIDE
                : R.plan.engine == LzEngine::block1 ? PROXSDP_LZ_ENGINE_BLOCK1 : PROXSDP_LZ_ENGINE_STEP;
        info[4] = R.split_cycle ? 1 : 0; info[5] = R.first_speculated ? 1 : 0; info[6] = R.merge_on_device ? 1 : 0;
        info[7] = R.split_ready ? 1 : 0;
        const size_t row = (size_t)c * cols;
        for (int k = kfirst; k < Kend; ++k) { t.alphas[row + k] = rec.al[k]; t.betas[row + k] = rec.be[k]; }
        for (int j = 0; j < kfirst; ++j) { t.D[row + j] = R.T[(size_t)j * R.ld + j]; t.f[row + j] = R.T[(size_t)j * R.ld + kfirst]; }
        PX_HIP(hipMemcpyAsync(t.V + row * npad, W.V.p, (size_t)cols * npad * sizeof(double), hipMemcpyDeviceToHost, stream));
        PX_HIP(hipStreamSynchronize(stream));
        info[8] = 0; info[9] = 0;
        if (kfirst > 0 && R.plan.engine != LzEngine::block1) {
            // What the cycle was handed: the restart rotation once more, through rotate_launch, from what it read -- the basis
            // of the cycle before (in W.Z: lz_restart swapped the buffers) and its coefficients, still on the device
            // (DeviceMerge::Uall after a device merge, else W.U behind rotate()'s upload) -- into a buffer of its own.  The
            // cycle's columns 0 .. kfirst must still be these bits.  (k_lz_block1 rotates in its own prologue: not repeated.)
            filled(again, (size_t)cols * npad, t.sentinel, stream);          // (the whole of a basis buffer's columns, as W.Z has them)
            const double* Ud = R.merge_on_device ? W.dmerge.Uall.p : W.U.p;
            const int form = W.rot_form, launches = W.rot_launches;
            std::swap(W.V.p, W.Z.p);
            rotate_launch(W, R.K, Ud, kfirst, again.p, R.K, kfirst);
            std::swap(W.V.p, W.Z.p);
            W.rot_form = form; W.rot_launches = launches;
            again_h.resize((size_t)(kfirst + 1) * npad);
            again.download(again_h.data(), again_h.size(), stream);
            PX_HIP(hipStreamSynchronize(stream));
            const double* snap = t.V + row * npad;
            int differ = 0;
            for (size_t q = 0; q < again_h.size(); ++q) differ += std::memcmp(&again_h[q], &snap[q], sizeof(double)) != 0;
            info[8] = 1; info[9] = differ;
        }
        if (t.more) t.more(W, R, info);
        *t.cycles = ++c;
    };
    lz_observer = &observe;
    try { lanczos(W0, xp, t.nev, t.positive_part); } catch (...) { lz_observer = nullptr; throw; }
    lz_observer = nullptr;
    PX_HIP(hipStreamSynchronize(stream));
    PX_HIP(hipGetLastError());
}
inline void Solver::test_lanczos_cycles(proxsdp_lanczos_cycles& t, const double* xp, proxsdp_positive_part* pp) {
    const LzCycleSink out{t.nev, t.max_cycles, t.cols, t.ldv, PROXSDP_LZ_INFO, t.sentinel, t.info, t.V, t.alphas, t.betas,
                          t.D, t.f, &t.cycles, nullptr, pp != nullptr};
    if (pp) test_positive_part(*pp, out, xp, t.n);
    else test_observed_run(out, xp);
}

// The same run on the OPERATOR FORM (include/proxsdp_hip.h proxsdp_operator_cycles): the block is never given densely.  The
// support list goes through build_block_operator -- setup_support's own ELL / overflow construction --, its values into the
// support-value array, the factors where ritz_pairs_to_block leaves them (W.F from column F_first on, W.Flam), and the block is
// armed as project_block arms it.  The capi entry validated every index, rank and value.
inline void Solver::test_operator_cycles(proxsdp_operator_cycles& t, proxsdp_positive_part* pp) {
    EigWork& W = eig[0];
    const int n = W.n, npad = W.npad, rp = t.rp;
    ns = (int)t.ns;
    const std::vector<int> supp(t.support, t.support + ns);
    esv_d.alloc((size_t)2 * std::max(ns, 1)); esv_d.zero(stream);
    if (ns > 0) esv_d.upload(t.esv, (size_t)2 * ns, stream);
    PX_HIP(hipStreamSynchronize(stream));
    P.blocks.assign(1, BlockInfo{n, W.N, 0});
    use_support = true;
    build_block_operator(W, P.blocks[0], supp, 0, supp.size());
    if (!W.fop_ok) throw std::invalid_argument("operator cycles: a row wider than 32 entries needs lanczos_operator = 1 below side 6000");
    t.ell_w = W.ell_w;
    t.overflow_rows = W.ov.wr_ptr != nullptr ? (int32_t)W.wr_row.n : 0;
    if (t.f_first + rp > W.cap) { W.F.alloc((size_t)npad * (t.f_first + rp)); W.F.zero(stream); }
    if (rp > 0) {
        std::vector<double> h((size_t)npad * rp, 0.0);
        for (int j = 0; j < rp; ++j) std::copy(t.F + (size_t)j * n, t.F + (size_t)j * n + n, h.begin() + (size_t)j * npad);
        PX_HIP(hipMemcpyAsync(W.F.p + (size_t)t.f_first * npad, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        W.Flam.upload(t.lam, rp, stream);
        PX_HIP(hipStreamSynchronize(stream));                 // host vectors go out of scope
    }
    W.have_factors = t.no_factors == 0; W.xprev.sparse = t.no_factors != 0;
    W.F_first = t.f_first; W.F_r = rp;
    if (!fop_eligible(W, true)) throw std::logic_error("operator cycles: the block is not eligible for the operator form");
    W.use_fop = true;
    arm_fop(W);
    if (t.probe_v) {
        // ONE mat-vec launch on the records form, outside any run: E v, the records of Vp'v and the shares of v'Ev
        std::vector<double> h(npad, 0.0);
        std::copy(t.probe_v, t.probe_v + n, h.begin());
        DevBuf<double> vd(npad);
        vd.upload(h.data(), npad, stream);
        PX_HIP(hipStreamSynchronize(stream));
        W.lzrun.plan.fop_owner = false;
        launch_symv(W, nullptr, vd.p, false, nullptr);
        PX_HIP(hipGetLastError());
        W.ebuf.download(t.probe_ev, npad, stream);
        W.tpart.download(t.probe_tpart, (size_t)W.nt * dev::RLD, stream);
        W.apartf.download(t.probe_apart, W.nt, stream);
        PX_HIP(hipStreamSynchronize(stream));
    }
    long long launches = W.lst.symv_launches;
    LzCycleSink out{t.nev, t.max_cycles, t.cols, t.ldv, PROXSDP_OP_INFO, t.sentinel, t.info, t.V, t.alphas, t.betas, t.D, t.f, &t.cycles, nullptr};
    out.more = [&](EigWork& Wc, LzRun& R, int32_t* info) {
        // (the mat-vecs counted for this cycle, a speculated one where it is used: each is a k_fop / k_fop_finish launch or a
        // step of k_lz_block1<., true> while use_fop is set)
        info[10] = Wc.use_fop ? (int32_t)(Wc.lst.symv_launches - launches) : 0;
        launches = Wc.lst.symv_launches;
        info[11] = lz_fop_owner(Wc) ? 1 : 0;
        info[12] = !Wc.use_fop ? 0 : Wc.F_r <= 64 ? 1 : 2;
        info[13] = Wc.ell_w;
        info[14] = t.overflow_rows;
        info[15] = R.plan.engine == LzEngine::block1 ? (Wc.b1_ell_in_lds ? 1 : 0) : -1;
    };
    out.positive_part = pp != nullptr;
    // (a positive-part run's certificate runs while use_fop is still set, as in full_eig_by_lanczos)
    try {
        if (pp) test_positive_part(*pp, out, nullptr, t.n);
        else test_observed_run(out, nullptr);
    } catch (...) { W.use_fop = false; throw; }
    W.use_fop = false;
}

// ONE positive-part run through the observed driver and its per-call certificate (include/proxsdp_hip.h proxsdp_positive_part),
// in full_eig_by_lanczos's order: lanczos(W, xp, nev, true), then lanczos_certificate on the pairs the run left in W.Z / W.vals
// -- or on the caller's, put there.  `out` is the wrapped entry's sink (positive_part set), eig[0] was sized for t.ws_rank
// pairs; the capi entry validated every argument and prefilled the caller's arrays.
inline void Solver::test_positive_part(proxsdp_positive_part& t, const LzCycleSink& out, const double* xp, int n) {
    EigWork& W = eig[0];
    const int npad = W.npad, cap = W.cap;
    if (cap != t.cap || npad != out.ldv) throw std::logic_error("positive part: the workspace is not the one asked for");
    if (t.run) {
        const long long warm0 = W.lst.warm_starts;
        test_observed_run(out, xp);
        t.warm = W.lst.warm_starts > warm0 ? 1 : 0;
        t.converged = W.converged ? 1 : 0; t.count = W.count; t.numiter = (int32_t)W.numiter;
        std::copy(W.vals.begin(), W.vals.begin() + W.count, t.vals);
        if (W.count > 0) W.Z.download(t.Z, (size_t)npad * W.count, stream);
        PX_HIP(hipStreamSynchronize(stream));
    } else {
        // no run: its parameters and its plan alone (the certificate launches under the plan of the run it certifies)
        lz_init(W, W.lzrun, out.nev, true);
        lz_plan(W, W.lzrun, true);
    }
    if (t.cert_steps < 2) return;
    if (t.npos_in < 0 && !W.converged) return;             // (full_eig_by_lanczos certifies a converged run only)
    const int npos = t.npos_in >= 0 ? t.npos_in : W.count;
    t.npos = npos;
    t.posres = lanczos_posres();
    const bool fits = npos + t.cert_steps + 1 <= cap;
    std::vector<double> h, before;
    if (t.npos_in >= 0) {
        W.vals.assign(t.locked_vals, t.locked_vals + npos);
        W.count = npos;
        if (fits && npos > 0) {
            h.assign((size_t)npad * npos, 0.0);
            for (int j = 0; j < npos; ++j) std::copy(t.locked + (size_t)j * n, t.locked + (size_t)j * n + n, h.begin() + (size_t)j * npad);
            W.Z.upload(h.data(), h.size(), stream);
            PX_HIP(hipStreamSynchronize(stream));
        }
    }
    if (fits) {
        h.assign((size_t)npad * (cap - npos), out.sentinel);
        PX_HIP(hipMemcpyAsync(W.Z.p + (size_t)npos * npad, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        before.resize((size_t)npad * std::max(npos, 1));
        if (npos > 0) W.Z.download(before.data(), (size_t)npad * npos, stream);
        PX_HIP(hipStreamSynchronize(stream));
    }
    const std::vector<double> vals0 = W.vals;
    const long long mv0 = W.lst.cert_matvecs;
    double theta = 0.0, scale = 0.0;
    t.cert_ran = lanczos_certificate(W, xp, npos, t.cert_steps, theta, scale) ? 1 : 0;
    PX_HIP(hipStreamSynchronize(stream));
    PX_HIP(hipGetLastError());
    t.matvecs = W.lst.cert_matvecs - mv0;
    if (!fits) return;                                      // (refused by the function before its first launch)
    t.theta_max = theta; t.scale = scale;
    const LzRecBuf narrow = W.record(false);
    const LzRecord rec(narrow.host, narrow.ld);
    t.stop = rec.ctl.stop; t.kstop = rec.ctl.kstop;
    t.steps = rec.ctl.stop ? std::max(0, std::min(t.cert_steps, rec.ctl.kstop - npos)) : t.cert_steps;
    for (int k = npos; k < npos + t.cert_steps; ++k) { t.cert_alphas[k] = rec.al[k]; t.cert_betas[k] = rec.be[k]; }
    W.Z.download(t.basis, (size_t)npad * cap, stream);
    W.resid2.download(t.resid2, npad, stream);
    PX_HIP(hipStreamSynchronize(stream));
    int64_t differ = 0;
    for (size_t q = 0; q < (size_t)npad * npos; ++q) differ += std::memcmp(&before[q], &t.basis[q], sizeof(double)) != 0;
    if (W.vals.size() != vals0.size()) differ += (int64_t)std::max(W.vals.size(), vals0.size());
    else for (size_t q = 0; q < vals0.size(); ++q) differ += std::memcmp(&vals0[q], &W.vals[q], sizeof(double)) != 0;
    t.differ = differ;
}

// The support path's copy of the non-PSD tail x[start .. N) (include/proxsdp_hip.h proxsdp_tail_copy) through launch_tail_copy,
// on t.wgs workgroups whose residual slots are the whole buffer (no PSD block in front); xout and respart prefilled.
inline void Solver::test_tail_copy(proxsdp_tail_copy& t) {
    std::vector<double> h((size_t)std::max<int64_t>(t.N, 2 * (int64_t)t.wgs), t.sentinel);
    DevBuf<double> dxin(t.N), dxout(t.N);
    dxin.upload(t.xin, t.N, stream);
    dxout.upload(h.data(), t.N, stream);
    mask_d.alloc(t.mask_words); mask_d.upload(t.mask, t.mask_words, stream);
    respart_d.alloc((size_t)2 * t.wgs); respart_d.upload(h.data(), (size_t)2 * t.wgs, stream);
    PX_HIP(hipStreamSynchronize(stream));
    P.n = t.N; P.sdplen = t.start;
    tile_base.assign(1, 0);
    n_res_wg = t.wgs;
    rstride = t.wgs;
    launch_tail_copy(dxin.p, dxout.p);
    PX_HIP(hipGetLastError());
    dxout.download(t.xout, t.N, stream);
    respart_d.download(t.respart, (size_t)2 * t.wgs, stream);
    PX_HIP(hipStreamSynchronize(stream));
}

}  // namespace proxsdp
