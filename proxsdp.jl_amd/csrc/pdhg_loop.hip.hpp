// The PDHG loop itself: primal_step!, linesearch!/dual_step!, compute_residual!,
// compute_gap!, the stop / rank-update / adaptive-step logic and the exit path.
// Each function cites the reference lines it replaces.
#pragma once
#include "solver.hip.hpp"

namespace proxsdp {

constexpr int PSTRIDE = 2048;       // stride of one quantity in the partials buffer
constexpr int NQ = 16;

// pdhg.jl:634 (Mx = M x)
inline void Solver::spmv(const double* x, double* y) {
    spmv_sparse(x, y);                                   // all Q rows (zeros for the rows of a dense A)
    if (P.dense()) dense_mv(x, y, true);                 // rows [0, p)
}
inline void Solver::spmv_sparse(const double* x, double* y) {
    if (P.Q == 0) return;
    if (rs.csr_wave)
        hipLaunchKernelGGL(dev::k_spmv_csr_wave, dim3(ceil_div(P.Q, dev::NWAVE)), dim3(dev::TPB), 0, stream,
                           rs.csr_ptr.p, rs.csr_col.p, rs.csr_val.p, x, y, (int)P.Q, LONG_ROW);
    else
        hipLaunchKernelGGL(dev::k_spmv_csr_thread, dim3(ceil_div(P.Q, dev::TPB)), dim3(dev::TPB), 0, stream,
                           rs.csr_ptr.p, rs.csr_col.p, rs.csr_val.p, x, y, (int)P.Q, LONG_ROW);
    if (rs.n_seg > 0) {
        hipLaunchKernelGGL(dev::k_spmv_csr_seg, dim3(rs.n_seg), dim3(dev::TPB), 0, stream,
                           rs.seg_lo_d.p, rs.seg_hi_d.p, rs.csr_col.p, rs.csr_val.p, x, rs.segpart_d.p);
        hipLaunchKernelGGL(dev::k_spmv_seg_fin, dim3(ceil_div(rs.n_long, dev::TPB)), dim3(dev::TPB), 0, stream,
                           rs.long_row_d.p, rs.long_ptr_d.p, rs.n_long, rs.segpart_d.p, y);
    }
}
// rows of the row pointers rp with more than LONG_ROW entries -> segments of SPMV_SEG entries, into `to`
inline void Solver::setup_long_rows(RowState& to, const std::vector<int>& rp) {
    std::vector<int> lo, hi, rows, ptr{0};
    for (size_t r = 0; r + 1 < rp.size(); ++r) {
        if (rp[r + 1] - rp[r] <= LONG_ROW) continue;
        rows.push_back((int)r);
        for (int k = rp[r]; k < rp[r + 1]; k += dev::SPMV_SEG) { lo.push_back(k); hi.push_back(std::min(k + dev::SPMV_SEG, rp[r + 1])); }
        ptr.push_back((int)lo.size());
    }
    to.build_segments((int)lo.size(), (int)rows.size());
    if (to.n_seg == 0) return;
    to.seg_lo_d.upload(lo.data(), to.n_seg, stream); to.seg_hi_d.upload(hi.data(), to.n_seg, stream);
    to.long_row_d.upload(rows.data(), to.n_long, stream); to.long_ptr_d.upload(ptr.data(), to.n_long + 1, stream);
    PX_HIP(hipStreamSynchronize(stream));
}

// the cone tail's launches: 1x1 PSD blocks (one_off -> one_min), SOC projection and SOC gap (soc_off, soc_len -> soc_gap_d)
inline void Solver::launch_clamp_scalars(double* x, int cnt) {
    hipLaunchKernelGGL(dev::k_clamp_scalars, dim3(ceil_div(cnt, 256)), dim3(256), 0, stream, x, one_off.p, cnt, one_min.p);
}
inline void Solver::launch_soc_project(double* x, int nsoc) {
    hipLaunchKernelGGL(dev::k_soc_project, dim3(nsoc), dim3(dev::TPB), 0, stream, x, soc_off.p, soc_len.p);
}
inline void Solver::launch_soc_gap(const double* x, int nsoc) {
    hipLaunchKernelGGL(dev::k_soc_gap, dim3(nsoc), dim3(dev::TPB), 0, stream, x, soc_off.p, soc_len.p, soc_gap_d.p);
}
// xsave = x[S]; x[S] -= tau (M'y + c)[S] in place, and the support values of the update for the operator-form mat-vec
inline void Solver::launch_primal_update_S(double* x, double tau) {
    hipLaunchKernelGGL(dev::k_primal_update_S, dim3(ceil_div(std::max(ns, 1), dev::TPB)), dim3(dev::TPB), 0, stream,
                       x, supp_d.p, MtyS_cur.p, cS_d.p, tau, xsave_d.p, ns, esv_d.p);
}

// the non-PSD tail of x on the support path (k_tail_copy_res): its workgroups own the residual slots behind the blocks' tiles
inline void Solver::launch_tail_copy(const double* xin, double* xout) {
    hipLaunchKernelGGL(dev::k_tail_copy_res, dim3(n_res_wg - tile_base.back()), dim3(dev::TPB), 0, stream,
                       xin, xout, (long long)P.sdplen, (long long)P.n, mask_d.p,
                       respart_d.p + tile_base.back(), rstride);
}

// primal_step! (pdhg.jl:611-637)
inline void Solver::primal_step_dev() {
    // block-sharded solve: a shard whose projection fails (e.g. non-finite input) must still join this iteration's
    // collectives, or its peers wait in them for ever: the error is kept, a flag travels with the iteration's scalar
    // record (reduce_candidates), and every shard aborts after that reduce
    auto shard_guard = [&](auto&& project) {
        if (!sharded()) { project(); return; }
        try {
            if (opt.debug_fail_iteration > 0 && iter == opt.debug_fail_iteration)
                throw std::runtime_error("injected projection failure (options.debug_fail_iteration)");
            project();
        } catch (...) { shard_error = std::current_exception(); }
    };
    if (use_support) {
        // x_k (buffer xc) becomes the matrix to project IN PLACE on the support; the projection
        // is written to the other buffer, so off the support buffer xc still holds x_k = x_old
        double* xcur = xbuf[xc].p;
        double* xnew = xbuf[1 - xc].p;
        launch_primal_update_S(xcur, primal_step);
        std::fill(min_eig.begin(), min_eig.end(), 0.0);
        double t0 = now_s();
        shard_guard([&]() { project_blocks(big_blocks, xcur, xnew, true); });
        st.t_psd += now_s() - t0;
        if (P.sdplen < P.n) launch_tail_copy(xcur, xnew);
        spmv(xnew, rs.Mxbuf[1 - mxc].p);
        reduce_coupling(rs.Mxbuf[1 - mxc].p);
        return;
    }
    const double* xi = xbuf[xc].p;
    double* xo = xbuf[1 - xc].p;
    hipLaunchKernelGGL(dev::k_primal_update, dim3(grid_for(P.n)), dim3(dev::TPB), 0, stream,
                       xo, xi, Mtybuf[mtyc].p, c_d.p, primal_step, (long long)P.n);
    // the general path inside a block-sharded solve: a shard with an SOC, a 1x1 block or no PSD block at all
    if (sharded()) st.reserved_s[PROXSDP_STATS_SHARDED_GENERAL_ITERATIONS]++;
    shard_guard([&]() {
        if (!P.blocks.empty()) {
            double t0 = now_s();
            psd_projection(xo);
            st.t_psd += now_s() - t0;
        }
        if (!P.socs.empty()) launch_soc_project(xo, (int)P.socs.size());
    });
    spmv(xo, rs.Mxbuf[1 - mxc].p);
    reduce_coupling(rs.Mxbuf[1 - mxc].p);
}

// ---- linesearch! / dual_step! (pdhg.jl:532-609) + compute_residual! + compute_gap! (residuals.jl:2-71) on every vector path
constexpr int NSCAL = 11;   // scalars per candidate (NCAND of them, solver.hip.hpp): q0,q1 sums | q2,q3 max, q4 sum | q5..q8 max, q9,q10 sum

// the candidates' buffers: y_c (the row state's: zeroed), M'y_c (on the support, or every column), partials, the scalar record
inline void Solver::alloc_candidates() {
    rs.ycand_d.zero(stream);
    Mtycand_d.alloc((size_t)NCAND * batch_shape().mstride); Mtycand_d.zero(stream);
    bpart.alloc((size_t)NCAND * NSCAL * PSTRIDE); bpart.zero(stream);
    bscal.alloc(64); bscal.zero(stream);
    hbscal.assign(64, 0.0);
    hscal_pin.alloc(64);
    PX_HIP(hipStreamSynchronize(stream));
}

// block-sharded solve: every shard evaluated the same candidates on its own blocks / rows: combine their scalar records
// (always NCAND of them, whatever the batch width: the collective's message keeps one size)
inline void Solver::reduce_candidates(int nc) {
    if (!sharded()) return;
    std::vector<double> sums, maxs;
    for (int c = 0; c < NCAND; ++c) {
        const double* sc = hbscal.data() + NSCAL * c;
        for (int q : {0, 1, 4, 9, 10}) sums.push_back(c < nc ? sc[q] : 0.0);
        for (int q : {2, 3, 5, 6, 7, 8}) maxs.push_back(c < nc ? sc[q] : 0.0);
    }
    maxs.push_back(hbscal[NCAND * NSCAL]); maxs.push_back(hbscal[NCAND * NSCAL + 1]);
    maxs.push_back(convergedrank() ? 0.0 : 1.0);          // any shard not rank-converged
    bool below = false;
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) below = below || target_rank[idx] < P.blocks[idx].n;
    maxs.push_back(below ? 1.0 : 0.0);                    // any block with target_rank < side
    maxs.push_back(now_s() - time0);                      // one clock for the limits
    maxs.push_back(shard_error ? 1.0 : 0.0);              // a shard failed in this iteration's projection
    if (shard_error)                                      // (its own partials may be garbage: keep them finite)
        for (double& v : sums) if (!(v == v)) v = 0.0;
    reduce(sums, maxs);
    if (maxs.back() > 0.5) {
        if (shard_error) { std::exception_ptr e = shard_error; shard_error = nullptr; std::rethrow_exception(e); }
        throw PeerFailure("another shard of the block-sharded solve failed in this iteration");
    }
    size_t si = 0, mi = 0;
    for (int c = 0; c < NCAND; ++c) {
        double* sc = hbscal.data() + NSCAL * c;
        for (int q : {0, 1, 4, 9, 10}) sc[q] = sums[si++];
        for (int q : {2, 3, 5, 6, 7, 8}) sc[q] = maxs[mi++];
    }
    hbscal[NCAND * NSCAL] = maxs[mi++]; hbscal[NCAND * NSCAL + 1] = maxs[mi++];
    g_not_converged_rank = maxs[mi++] > 0.5;
    g_any_below_full = maxs[mi++] > 0.5;
    g_elapsed = maxs[mi++];
}

// ---- one batch of linesearch candidates: the launches (shared with the kernel-level test entry, test_trial_batch)
// the batch's launch shapes: one workgroup column per 256 entries of y (gq) and of the support or every column (gx), capped at
// PSTRIDE (the kernels stride over the rest); the candidates' slices of rs.ycand_d / Mtycand_d / bpart; and the one place that
// tells the vector paths apart for the batch (the support path keeps M'y on S in one buffer, which commit overwrites)
inline Solver::BatchShape Solver::batch_shape() const {
    BatchShape b;
    if (use_support) { b.supp = supp_d.p; b.cnt = ns; b.xold = xsave_d.p; b.cv = cS_d.p; b.mty_cur = b.mty_commit = MtyS_cur.p; }
    else { b.supp = nullptr; b.cnt = P.n; b.xold = xbuf[xc].p; b.cv = c_d.p; b.mty_cur = Mtybuf[mtyc].p; b.mty_commit = Mtybuf[1 - mtyc].p; }
    b.gq = std::min(PSTRIDE, grid_for(std::max<int64_t>(P.Q, 1)));
    b.gx = std::min(PSTRIDE, grid_for(std::max<long long>(b.cnt, 1)));
    b.cstride = (long long)NSCAL * PSTRIDE;
    b.ystride = std::max<int64_t>(P.Q, 1);
    b.mstride = std::max<long long>(b.cnt, 1);
    return b;
}
// residual / gap reductions of candidates c0 .. c0 + nc - 1 (their partials land in the records 0 .. nc - 1)
inline void Solver::batch_residuals(const dev::TrialBatch& tb, int nc, int c0, double xold_coef) {
    const BatchShape b = batch_shape();
    const double* yc0 = rs.ycand_d.p + (size_t)c0 * b.ystride;
    const double* mc0 = Mtycand_d.p + (size_t)c0 * b.mstride;
    // (outside a block-sharded solve the general path's residuals have never taken the row weights that k_dual_trial_batch
    // gets on both paths: kept as it is, and with it that solve's bits; inside one, b'y and h'y count a coupling row once)
    const double* roww = (b.supp != nullptr || general_row_weights) ? roww_d.p : nullptr;
    hipLaunchKernelGGL(b.supp != nullptr ? dev::k_residual_xy<true> : dev::k_residual_xy<false>,
                       dim3(std::max(b.gx, b.gq), nc, 2), dim3(dev::TPB), 0, stream,
                       xbuf[1 - xc].p, b.supp, b.cnt, b.xold, xold_coef, mc0, b.mstride, b.mty_cur, b.cv, b.gx,
                       yc0, b.ystride, rs.ybuf[yc].p, rs.Mxbuf[1 - mxc].p, rs.Mxbuf[mxc].p, rs.bh_d.p, (int)P.p, (int)P.Q, b.gq,
                       tb, bpart.p, PSTRIDE, b.cstride, roww);
}
// y+, M'y+ and their norms for nc candidates, then their residuals
// (the vector paths differ only in the view batch_shape() gives and, for a dense M, in the M'y+ product)
inline void Solver::batch_evaluate(const dev::TrialBatch& tb, int nc, double xold_coef) {
    const BatchShape b = batch_shape();
    const int gq = b.gq;
    const long long cstride = b.cstride, ystride = b.ystride;
    hipLaunchKernelGGL(dev::k_dual_trial_batch, dim3(gq, nc), dim3(dev::TPB), 0, stream,
                       rs.ybuf[yc].p, rs.Mxbuf[1 - mxc].p, rs.Mxbuf[mxc].p, rs.bh_d.p, (int)P.p, (int)P.Q, tb,
                       rs.ycand_d.p, ystride, bpart.p, cstride, roww_d.p);
    batch_mty(tb, nc);
    batch_residuals(tb, nc, 0, xold_coef);
}
// M'y_c of the candidates in rs.ycand_d + |M'y_c - M'y_old|^2 partials
inline void Solver::batch_mty(const dev::TrialBatch& tb, int nc) {
    const BatchShape b = batch_shape();
    if (b.supp == nullptr && P.dense())
        dense_mtv(nc, rs.ycand_d.p, b.ystride, true, Mtycand_d.p, b.mstride, b.mty_cur, nullptr, bpart.p + PSTRIDE, b.cstride, !tb.plain);
    else
        hipLaunchKernelGGL(b.supp != nullptr ? dev::k_spmvT_batch<true> : dev::k_spmvT_batch<false>,
                           dim3(b.gx, nc), dim3(dev::TPB), 0, stream,
                           rs.csc_ptr.p, rs.csc_row.p, rs.csc_val.p, b.supp, b.cnt, rs.ycand_d.p, b.ystride,
                           Mtycand_d.p, b.mstride, b.mty_cur, bpart.p + PSTRIDE, b.cstride, tb.plain);
}
// the scalar record: NSCAL per candidate, then (support path) the two off-support residual maxima that the fused
// reconstruction reduced -- independent of the candidate, combined by two extra workgroups.  Returns the record.
inline const double* Solver::batch_read_back(int nc) {
    const BatchShape b = batch_shape();
    const int gq = b.gq, gx = b.gx;
    unsigned long long ismax = 0;
    for (int c = 0; c < nc; ++c) ismax |= 0x1ECull << (NSCAL * c);      // bits 2,3,5,6,7,8 of every candidate
    if (use_support) {
        // (measured, tools/_ab in round 5: letting this kernel write its scalars straight into pinned host memory -- as the
        // small-model path does -- costs the rank-63 iteration 3 %: a kernel that stores to host memory ends with a system-scope
        // release, and behind the reconstruction that means writing 64 MB of dirty L2 lines back first)
        hipLaunchKernelGGL(dev::k_combine_multi, dim3(nc * NSCAL + 2), dim3(dev::TPB), 0, stream,
                           (const double*)bpart.p, PSTRIDE, std::max(gq, gx), ismax, bscal.p, nc * NSCAL,
                           (const double*)respart_d.p, rstride, n_res_wg, bscal.p + NCAND * NSCAL);
        PX_HIP(hipMemcpyAsync(hbscal.data(), bscal.p, (NCAND * NSCAL + 2) * sizeof(double), hipMemcpyDeviceToHost, stream));
        wait_stream();
        reduce_candidates(nc);
        return hbscal.data();
    }
    // small models: the scalars go STRAIGHT into pinned host memory (no copy launch: 6 us of a 60 us iteration); larger ones keep
    // the copy (a kernel that stores to host memory ends with a system-scope release of everything the iteration left dirty)
    const bool zc = zero_copy_small();
    hipLaunchKernelGGL(dev::k_combine_multi, dim3(nc * NSCAL), dim3(dev::TPB), 0, stream,
                       (const double*)bpart.p, PSTRIDE, std::max(gq, gx), ismax, zc ? hscal_pin.p : bscal.p, nc * NSCAL,
                       (const double*)nullptr, 0, 0, (double*)nullptr);
    if (!zc) PX_HIP(hipMemcpyAsync(hscal_pin.p, bscal.p, NCAND * NSCAL * sizeof(double), hipMemcpyDeviceToHost, stream));
    wait_stream();
    if (!sharded()) return hscal_pin.p;
    // block-sharded solve: the host must see ONE combined record, so the pinned one is copied and reduced in hbscal.  The two
    // off-support slots are global after the reduce (a support-path shard of the same solve fills them); this path's slots 2
    // and 3 cover every entry already, so it contributes 0 to them
    std::copy(hscal_pin.p, hscal_pin.p + (size_t)nc * NSCAL, hbscal.begin());
    hbscal[NCAND * NSCAL] = hbscal[NCAND * NSCAL + 1] = 0.0;
    reduce_candidates(nc);
    return hbscal.data();
}

// Up to NCAND consecutive step-size candidates tau, 0.75 tau, 0.75^2 tau are evaluated by ONE batch of launches -- y+, M'y+ and
// their norms, then the residual / gap reductions, pure reductions over each candidate's y and M'y -- and ONE read-back; the host
// takes the first candidate the reference's loop would have accepted.  Per candidate the arithmetic is that of a batch of one, so
// the batch width changes no bit.  line_search_flag = false: ONE plain candidate, dual_step! (pdhg.jl:584-609) -- y+ = y +
// sigma (2 Mx - Mx_old) with the solver's own dual_step, taken as it is; primal_step, dual_step and theta are left alone.
// Returns the accepted candidate's scalar record.
inline const double* Solver::linesearch_and_residuals() {
    const int ncmax = opt.general_batch != 0 ? NCAND : 1;
    const double xold_coef = (iter == 1 && opt.advanced_initialization && !start_active) ? 0.0 : 1.0;   // x_old = 0 at k = 1 (a warm start has x_old = x)
    const double* rec = nullptr;
    auto commit = [&](int c) {                           // y <- y_c, M'y <- M'y_c (one launch)
        const BatchShape b = batch_shape();
        hipLaunchKernelGGL(dev::k_copy2, dim3(grid_for((long long)P.Q + b.cnt)), dim3(dev::TPB), 0, stream,
                           rs.ybuf[1 - yc].p, (const double*)(rs.ycand_d.p + (size_t)c * b.ystride), (long long)P.Q,
                           b.mty_commit, (const double*)(Mtycand_d.p + (size_t)c * b.mstride), b.cnt);
    };
    const bool ls = opt.line_search_flag;
    if (ls) primal_step = primal_step * std::sqrt(1.0 + theta);
    int trials = 0;
    const double* s_acc = nullptr;
    while (s_acc == nullptr) {
        dev::TrialBatch tb{};
        double tau_c = primal_step;
        int nc = 0;
        for (; ls && nc < ncmax && trials + nc < opt.max_linsearch_steps; ++nc) {
            tb.tau[nc] = tau_c;
            tb.theta[nc] = tau_c / primal_step_old;
            tb.bt[nc] = beta * tau_c;
            tb.sigma[nc] = beta * tau_c;
            tau_c *= opt.linsearch_decay;
        }
        if (!ls) { nc = 1; tb.tau[0] = primal_step; tb.theta[0] = 1.0; tb.bt[0] = dual_step; tb.sigma[0] = dual_step; tb.plain = 1; }
        tb.nc = nc;
        batch_evaluate(tb, nc, xold_coef);
        rec = batch_read_back(nc);
        for (int c = 0; c < nc && s_acc == nullptr; ++c) {
            ++trials;
            const double* sc = rec + NSCAL * c;
            if (ls) {
                primal_step = tb.tau[c];
                theta = tb.theta[c];
                const double y_norm = std::sqrt(sc[0]), Mty_norm = std::sqrt(sc[1]);
                if (debug && iter <= 5 && trials <= 6)
                    std::fprintf(stderr, "[dbg] it %lld trial %d tau %.6e theta %.6e y_norm %.6e Mty_norm %.6e\n",
                                 iter, trials, primal_step, theta, y_norm, Mty_norm);
                const bool ok = std::sqrt(beta) * primal_step * Mty_norm <= opt.delta * y_norm;
                if (!ok && trials < opt.max_linsearch_steps) { primal_step = tb.tau[c] * opt.linsearch_decay; continue; }
                if (!ok) {
                    // reference quirk (pdhg.jl:545-569): max_linsearch_steps exhausted -> the step is decayed once more while
                    // the last trial's y / M'y are kept, and compute_residual! / compute_gap! then run with THAT primal_step and
                    // dual_step: candidate c's residual scalars are evaluated again with the final steps (rare: one more batch)
                    primal_step *= opt.linsearch_decay;
                    dev::TrialBatch t1{};
                    t1.nc = 1; t1.tau[0] = primal_step; t1.theta[0] = theta; t1.bt[0] = beta * primal_step;
                    t1.sigma[0] = beta * primal_step;
                    batch_residuals(t1, 1, c, xold_coef);
                    rec = batch_read_back(1);
                    sc = rec;                            // (its two norms, slots 0 and 1, are not read any more)
                }
            }
            s_acc = sc;
            commit(c);
        }
    }
    primal_step_old = primal_step;
    if (ls) dual_step = beta * primal_step;
    st.linesearch_trials += trials;
    last_trials = trials;
    return s_acc;
}

// compute_residual! + compute_gap! (residuals.jl:2-71) from the accepted candidate's scalar record, then the *_old rotation
// (:65-68) as index flips instead of four vector copies
inline void Solver::record_residuals(const double* s) {
    if (debug && iter <= 5)
        std::fprintf(stderr, "[dbg] it %lld res: %.6e %.6e cx %.6e | %.6e %.6e eq %.6e in %.6e by %.6e hy %.6e\n",
                     iter, s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10]);
    // (+ the off-support maxima: global after the reduce of a block-sharded solve, so every shard folds them, whatever its own
    // path -- or a support-path shard and a general-path shard of one solve would compute different residuals)
    const bool fold = use_support || sharded();
    const double m0 = fold ? std::max(s[2], hbscal[NCAND * NSCAL]) : s[2];
    const double m1 = fold ? std::max(s[3], hbscal[NCAND * NSCAL + 1]) : s[3];
    const double pres = std::sqrt(g_n) * m0 / std::max({m1, g_norm_b, g_norm_h, 1.0});
    const double dres = std::sqrt(g_Q) * s[5] / std::max({s[6], g_norm_c, 1.0});
    h_pres.at(iter) = pres;
    h_dres.at(iter) = dres;
    h_comb.at(iter) = std::max(pres, dres);
    if (g_p > 0) equa_feasibility = s[7] / (1.0 + g_norm_b);
    if (g_m > 0) ineq_feasibility = s[8] / (1.0 + g_norm_h);
    h_feas.at(iter) = std::max(equa_feasibility, ineq_feasibility);
    const double po = s[4];
    double d_o = 0.0;
    if (g_p > 0) d_o -= s[9];
    if (g_m > 0) d_o -= s[10];
    h_pobj.at(iter) = po;
    h_dobj.at(iter) = d_o;
    h_gap.at(iter) = std::fabs(po - d_o) / (1.0 + std::fabs(po) + std::fabs(d_o));
    xc = 1 - xc; yc = 1 - yc; mxc = 1 - mxc;
    if (!use_support) mtyc = 1 - mtyc;                   // (the support path keeps M'y on S in one buffer, updated by commit)
}

// convergedrank (residuals.jl:88-101)
inline bool Solver::convergedrank() const {
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
        if (!(P.blocks[idx].n < opt.min_size_krylov_eigs ||
              target_rank[idx] > opt.max_target_rank_krylov_eigs || min_eig[idx] < opt.tol_psd))
            return false;
    }
    return true;
}

// soc_convergence (residuals.jl:73-86)
inline bool Solver::soc_convergence() {
    bool open = false;                                   // some gap >= tol_soc
    if (!P.socs.empty()) {
        launch_soc_gap(xbuf[xc].p, (int)P.socs.size());
        std::vector<double> g(P.socs.size());
        soc_gap_d.download(g.data(), g.size(), stream);
        PX_HIP(hipStreamSynchronize(stream));
        for (double v : g) open = open || v >= opt.tol_soc;
    }
    // block-sharded solve: the answer is the model's.  All shards arrive here together (the conditions in front of this call
    // are built from reduced scalars), SOC-free ones included: one extra scalar reduce
    if (sharded()) {
        std::vector<double> sums, maxs = {open ? 1.0 : 0.0};
        reduce(sums, maxs);
        open = maxs[0] > 0.5;
    }
    return !open;
}

// certificate_parameters (pdhg.jl:670-676)
inline void Solver::certificate_parameters() {
    certificate_search_min_iter = iter + 2 * opt.convergence_window + iter / 5 + 1000;
    certificate_search = true;
    time_limit *= 1.1;
    max_iter_local = max_iter_local + max_iter_local / 10;
}

// the rank-update rule shared by pdhg.jl:270-280 and :294-301
inline void Solver::bump_rank(int idx) {
    if (current_rank[idx] + opt.rank_slack >= target_rank[idx]) {
        if (min_eig[idx] > opt.tol_psd) {
            long long side = P.blocks[idx].n;
            if (opt.rank_increment == 0)
                target_rank[idx] = std::min<long long>(opt.rank_increment_factor * target_rank[idx], side);
            else
                target_rank[idx] = std::min<long long>(opt.rank_increment_factor + target_rank[idx], side);
        }
    }
}

// lambda_min of smat(dc_k) for the dual-cone block of PSD cone idx (side >= 2).  fill(tmp, negated) puts the packed block -- or
// minus it -- into the device buffer tmp on the solver's stream: from a host vector (dual_feas_host) or by a kernel
// (cache_solution_device).
// psd_vec_to_square(v, a, cones, sqrt(2)): off-diagonals / sqrt(2), i.e. smat(dc).
// The reference takes minimum(eigen!(...)) of the full spectrum (pdhg.jl:685, one
// O(n^3) dsyevr inside SolveTimeSec); only lambda_min is used, so for Lanczos-sized
// blocks it is computed as -lambda_max(-smat(dc)) with the projection's own Lanczos
// (a few hundred mat-vecs), falling back to the dense eigensolver if that does not
// converge.  This also keeps rocSOLVER's 3-5 s one-off code-object load out of
// solves that never take the full_eig! path.
template <typename Fill>
inline double Solver::dual_block_min_eig(size_t idx, Fill&& fill) {
    const BlockInfo& B = P.blocks[idx];
    EigWork& W = eig[idx];
    DevBuf<double> tmp(B.N);
    double mn = 0.0;
    bool have_mn = false;
    if (B.n > opt.min_size_krylov_eigs && opt.eigsolver != 1 && W.cap >= 26 && krylovdim_fits(1)) {
        fill(tmp.p, true);
        const proxsdp_stats keep_st = W.lst;
        const long long keep_mv = W.mv_iter;
        const int keep_prev = W.prev_numiter, keep_num = W.numiter;
        W.use_fop = false;
        lanczos(W, tmp.p, 1);
        if (W.converged && W.converged_eigs >= 1 && !W.vals.empty()) { mn = -W.vals[0]; have_mn = true; }
        const long long mv = W.lst.lanczos_matvecs - keep_st.lanczos_matvecs;
        W.lst = keep_st;                               // exit-path work is not a projection
        st.exit_matvecs += mv;
        W.mv_iter = keep_mv;
        W.prev_numiter = keep_prev; W.numiter = keep_num;
        PX_HIP(hipStreamSynchronize(stream));          // (the host vector behind fill may go now)
    }
    if (!have_mn) {
        fill(tmp.p, false);
        std::vector<double> D;
        full_eig_values(W, tmp.p, dev::INV_SQRT2, false, D);
        mn = D[0];
        for (double v : D) mn = std::min(mn, v);
    }
    return mn;
}

// get_duals + dual_feas + cone_feas (pdhg.jl:678-732) on host vectors; the
// dual-cone eigenvalues come from the device (rocSOLVER, values only).
inline double Solver::dual_feas_host(const std::vector<double>& y, const std::vector<double>& cvec,
                                     std::vector<double>* dual_eq, std::vector<double>* dual_in,
                                     std::vector<double>* dual_cone_out) {
    std::vector<double> dc(cvec);
    if (P.dense()) {                                          // c + M'y with the caller's (unscaled) M
        DevBuf<double> yd(std::max<int64_t>(P.Q, 1)), cd(P.n), od(P.n);
        yd.upload(y.data(), P.Q, stream); cd.upload(cvec.data(), P.n, stream);
        dense_mtv(1, yd.p, 0, false, od.p, 0, nullptr, cd.p, nullptr, 0, false);
        od.download(dc.data(), P.n, stream);
        PX_HIP(hipStreamSynchronize(stream));
    }
    for (int64_t k = 0; k < P.n; ++k) {
        double acc = 0.0;
        for (int64_t q = P.colptr[k]; q < P.colptr[k + 1]; ++q) acc += P.val_orig[q] * y[P.rowidx[q]];
        dc[k] += acc;
        if (P.offdiag[k]) dc[k] /= 2.0;                       // fix_diag_scaling(dual_cone, cones, 2.0)
    }
    double ineq_viol = 0.0;
    if (P.m > 0) {
        double mn = y[P.p];
        for (int64_t i = 0; i < P.m; ++i) mn = std::min(mn, y[P.p + i]);
        ineq_viol = -std::min(0.0, mn);
    }
    double sdp_viol = 0.0;
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
        const BlockInfo& B = P.blocks[idx];
        if (B.n == 1) {
            sdp_viol = std::max(sdp_viol, -std::min(0.0, dc[B.off]));
        } else {
            std::vector<double> stage;                         // (outlives the upload: the helper synchronises)
            const double mn = dual_block_min_eig(idx, [&](double* tmp, bool negated) {
                stage.assign(dc.begin() + B.off, dc.begin() + B.off + B.N);
                if (negated) for (double& v : stage) v = -v;
                PX_HIP(hipMemcpyAsync(tmp, stage.data(), (size_t)B.N * sizeof(double), hipMemcpyHostToDevice, stream));
            });
            sdp_viol = std::max(sdp_viol, -std::min(0.0, mn));
        }
    }
    for (const SocInfo& S : P.socs) {
        double ss = 0.0;
        for (int i = 1; i < S.len; ++i) ss += dc[S.off + i] * dc[S.off + i];
        sdp_viol = std::max(sdp_viol, -std::min(0.0, dc[S.off] - std::sqrt(ss)));
    }
    double zero_viol = 0.0;
    for (int64_t k = P.conelen; k < P.n; ++k) zero_viol = std::max(zero_viol, std::fabs(dc[k]));
    if (dual_eq) dual_eq->assign(y.begin(), y.begin() + P.p);
    if (dual_in) dual_in->assign(y.begin() + P.p, y.end());
    if (dual_cone_out) *dual_cone_out = std::move(dc);
    return std::max({sdp_viol, ineq_viol, zero_viol});
}

// what a snapshot leaves beside its vectors: the scalar fields of the result, and the workspaces' bookkeeping
inline void Solver::finish_snapshot(double dfeas) {
    harvest_small_ranks();
    long long fr = 0;
    for (long long r : current_rank) fr += r;
    if (sharded()) {                         // dual feasibility and rank over all shards
        std::vector<double> sums = {(double)fr}, maxs = {dfeas};
        reduce(sums, maxs);
        fr = (long long)std::llround(sums[0]);
        dfeas = maxs[0];
    }
    res.status = stop_reason;
    merge_block_stats();
    // (a caller who forces equilibration gets the reference's aliased -- not contractive -- scaling iteration by default: say so)
    std::snprintf(res.status_string, sizeof(res.status_string), "%s%s%s", stop_reason_string.c_str(),
                  st.dense_truncated_projections > 0 ? " [Krylov dimension > 255: dense eigensolver served those projections]" : "",
                  (P.equilibrated && opt.equilibration_reference_aliasing) ? " [equilibration: the reference's aliased scaling, equilibration_reference_aliasing = 1]" : "");
    res.primal_residual = equa_feasibility;
    res.dual_residual = ineq_feasibility;
    res.objval = h_pobj.at(iter);
    res.dual_objval = h_dobj.at(iter);
    res.gap = h_gap.at(iter);
    res.iter = iter;
    res.final_rank = (int32_t)fr;
    res.primal_feasible_user_tol = h_feas.at(iter) <= opt.tol_feasibility;
    res.dual_feasible_user_tol = dfeas <= opt.tol_feasibility_dual;
    res.dual_feasibility = dfeas;
    res.certificate_found = certificate_found;
    res.result_count = 1;
    res.time = now_s() - time0;
    have_snapshot = true;
    // x was rescaled IN PLACE above (the reference quirk, pdhg.jl:749-755).  When a certificate
    // search continues from here, the operator-form factors F diag(Flam) F' still describe the
    // UNscaled iterate: drop them so the next projection reads the (rescaled) packed buffer, as the
    // fused residual and the dense / full-eig paths do.
    for (EigWork& W : eig) { W.have_factors = false; W.xprev.sparse = false; W.ritz_ok = false; }
}

// cache_solution (pdhg.jl:745-787).  NB the reference rescales pair.x IN PLACE
// (fix_diag_scaling on pair.x, :749); when a certificate search continues after
// this snapshot the iterate stays rescaled -- reproduced here on the device.
inline void Solver::cache_solution(const std::vector<double>& cvec) {
    double t0 = now_s();
    exit_rescale_iterate();                                  // (exit_device.hip.hpp: the two exit paths share it)
    std::vector<double> x(P.n), y(P.Q);
    xbuf[xc].download(x.data(), P.n, stream);
    rs.ybuf[yc].download(y.data(), P.Q, stream);
    PX_HIP(hipStreamSynchronize(stream));
    std::vector<double> slack(P.Q, 0.0);
    if (P.dense() && P.p > 0) {                              // A x with the caller's (unscaled) dense A
        DevBuf<double> sd(P.p);
        dense_mv(xbuf[xc].p, sd.p, false);
        sd.download(slack.data(), P.p, stream);
        PX_HIP(hipStreamSynchronize(stream));
    }
    for (int64_t k = 0; k < P.n; ++k) {
        const double xk = x[k];
        for (int64_t q = P.colptr[k]; q < P.colptr[k + 1]; ++q) slack[P.rowidx[q]] += P.val_orig[q] * xk;
    }
    if (!coup_rows.empty()) {                                 // M x of a coupling row: sum of the shards' partials
        std::vector<double> part_(coup_rows.size());
        for (size_t k = 0; k < coup_rows.size(); ++k) part_[k] = slack[coup_rows[k]];
        reduce_vec_host(part_);
        for (size_t k = 0; k < coup_rows.size(); ++k) slack[coup_rows[k]] = part_[k];
    }
    // the factors of this snapshot's PSD blocks, before the lambda_min Lanczos below reuses the blocks' workspaces
    if (req.factors_out) {
        std::vector<double> one_vals(P.blocks.size(), 0.0);
        for (size_t idx = 0; idx < P.blocks.size(); ++idx) if (P.blocks[idx].n == 1) one_vals[idx] = x[P.blocks[idx].off];
        extract_factors(one_vals);
    }
    std::vector<double> deq, din, dcone;
    const double dfeas = dual_feas_host(y, cvec, &deq, &din, &dcone);
    if (res.primal)    for (int64_t i = 0; i < P.n; ++i) res.primal[i] = x[P.inv[i]];
    if (res.dual_cone) for (int64_t i = 0; i < P.n; ++i) res.dual_cone[i] = dcone[P.inv[i]];
    if (res.dual_eq)   for (int64_t i = 0; i < P.p; ++i) res.dual_eq[i] = deq[i];
    if (res.dual_in)   for (int64_t i = 0; i < P.m; ++i) res.dual_in[i] = din[i];
    if (res.slack_eq)  for (int64_t i = 0; i < P.p; ++i) res.slack_eq[i] = slack[i] - P.b_orig[i];
    if (res.slack_in)  for (int64_t i = 0; i < P.m; ++i) res.slack_in[i] = slack[P.p + i] - P.h_orig[i];
    finish_snapshot(dfeas);
    st.exit_time += now_s() - t0;
}

// The low-rank factors of the PSD blocks of the snapshot cache_solution is taking (proxsdp_hip_solve_factored): for cone k
// the positive eigenpairs of the block exactly as it sits in xbuf[xc] -- plain entries in the caller's scale, what is
// downloaded into res->primal (one_vals[k]: that entry of a 1x1 cone k, all the host needs of the iterate).
// Where the block still IS the reconstruction of the last projection's Ritz pairs (the operator form's factors F / Flam, or the pairs a converged Krylov projection left in Z / vals) those pairs
// are handed out: a gather and a download, no eigensolve.  Any other block of side >= 2 -- full_eig! engines, equilibrated
// solves (the rescale by D is not a congruence the pairs survive), a snapshot taken before any projection -- gets one
// dsyevd of the block, pairs with lambda > 0 kept.  Either way the cap[k] largest pairs go out, descending, and
// k_factor_residual measures them against the block: resid reports what the pairs miss, truncation included.
inline void Solver::extract_factors(const std::vector<double>& one_vals) {
    proxsdp_psd_factors& F = *req.factors_out;
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
        const BlockInfo& B = P.blocks[idx];
        const int64_t cap = F.cap[idx];
        double* vout = F.vectors + F.vec_ptr[idx];
        double* lout = F.values + F.val_ptr[idx];
        F.rank[idx] = 0; F.rank_found[idx] = 0; F.source[idx] = PROXSDP_FACTOR_NONE;
        F.resid[idx] = 0.0; F.xnorm[idx] = 0.0;
        if (cap <= 0) continue;                               // nothing wanted for this cone: nothing computed
        if (B.n == 1) {
            const double xv = one_vals[idx];
            F.xnorm[idx] = std::fabs(xv);
            if (xv > 0.0) { vout[0] = 1.0; lout[0] = xv; F.rank[idx] = 1; F.rank_found[idx] = 1; }
            else F.resid[idx] = std::fabs(xv);
            continue;
        }
        EigWork& W = eig[idx];
        const int n = B.n;
        const double* xp = xbuf[xc].p + B.off;
        const double* Vsrc = nullptr;
        int ldv = 0;
        std::vector<double> lam;                              // candidate pairs: lam[c] belongs to column c of Vsrc
        if (!P.equilibrated && (W.have_factors || W.ritz_ok)) {
            F.source[idx] = PROXSDP_FACTOR_RITZ;
            ldv = W.npad;
            if (W.have_factors) {
                Vsrc = W.prev_factors().V;
                lam.resize(W.F_r);
                if (W.F_r > 0) { W.Flam.download(lam.data(), W.F_r, stream); PX_HIP(hipStreamSynchronize(stream)); }
            } else {
                Vsrc = W.Z.p + (size_t)W.ritz_first * W.npad;
                lam.assign(W.vals.begin() + W.ritz_first, W.vals.begin() + W.ritz_first + W.ritz_r);
            }
        } else {
            F.source[idx] = PROXSDP_FACTOR_EIG;
            full_eig_values(W, xp, 1.0, true, lam);           // (plain entries: no off-diagonal factor)
            Vsrc = W.A.p; ldv = n;
        }
        // the positive pairs, largest first (KrylovKit's pairs come descending, ARPACK's and dsyevd's ascending)
        std::vector<int> order;
        for (int c = 0; c < (int)lam.size(); ++c) if (lam[c] > 0.0) order.push_back(c);
        std::stable_sort(order.begin(), order.end(), [&lam](int a, int b) { return lam[a] > lam[b]; });
        const int found = (int)order.size();
        const int k = (int)std::min<int64_t>(cap, found);
        F.rank_found[idx] = found; F.rank[idx] = k;
        if (k > 0) {
            if (fac_V.n < (size_t)n * k) fac_V.alloc((size_t)n * k);
            if (fac_lam.n < (size_t)k) fac_lam.alloc(k);
            for (int j = 0; j < k; ++j) {
                lout[j] = lam[order[j]];
                PX_HIP(hipMemcpyAsync(fac_V.p + (size_t)j * n, Vsrc + (size_t)order[j] * ldv, (size_t)n * sizeof(double),
                                      hipMemcpyDeviceToDevice, stream));
            }
            fac_lam.upload(lout, k, stream);
            fac_V.download(vout, (size_t)n * k, stream);
        }
        double r2 = 0.0, x2 = 0.0;
        factor_residual(xp, n, fac_V.p, n, fac_lam.p, k, r2, x2);
        F.resid[idx] = std::sqrt(r2); F.xnorm[idx] = std::sqrt(x2);
    }
}

// ---- dense constraint matrix (proxsdp_problem.M_dense; kernels.hip.hpp "Dense constraint matrix")
inline void Solver::upload_dense() {
    if (Md != nullptr) return;
    const size_t cnt = (size_t)P.p * (size_t)P.n;
    if (P.Mdense_on_device) {
        Md = P.Mdense;                                   // borrowed, read-only
    } else {
        Md_own.alloc(std::max<size_t>(cnt, 1));
        const size_t chunk = (size_t)1 << 27;            // 1 GiB of doubles per copy
        for (size_t o = 0; o < cnt; o += chunk)
            PX_HIP(hipMemcpy(Md_own.p + o, P.Mdense + o, std::min(chunk, cnt - o) * sizeof(double), hipMemcpyHostToDevice));
        Md = Md_own.p;
    }
    offdiag_d.alloc(P.n);
    offdiag_d.upload(P.offdiag.data(), P.n, stream);
    // M x: row groups x column slices; enough workgroups to fill 256 CUs several times over
    const int rg = ceil_div((int)std::max<int64_t>(P.p, 1), DMV_ROWS);
    dmv_slices = std::max(1, std::min(64, ceil_div(2048, rg)));
    const long long chunks = ((long long)P.n + dev::TPB * DMV_UNR - 1) / (dev::TPB * DMV_UNR);
    dmv_slices = (int)std::min<long long>(dmv_slices, std::max<long long>(chunks, 1));
    dmv_qpad = (int)std::max<int64_t>(P.p, 1);
    dmv_part.alloc((size_t)dmv_slices * dmv_qpad);
}

// Equilibration on a dense A (the part prepare() deferred): ONE pass over the borrowed matrix for the row sums and the
// extrema, then the limit check and the scaling iteration on the host (O(Q) per iteration), the scale vectors of the
// dense products, and ||E A D S||_F^2 = d^2 sum_i e_i^2 R'_i.  Runs before anything reads P.b / P.h / P.c / P.val.
inline void Solver::setup_dense_scaling() {
    if (!P.equil_deferred) return;
    upload_dense();
    std::vector<double> out((size_t)2 * dmv_qpad + 2, 0.0);
    if (P.p > 0) {
        const int rg = ceil_div((int)P.p, DMV_ROWS);
        const int nwg = rg * dmv_slices;
        DevBuf<double> spart((size_t)2 * dmv_slices * dmv_qpad), smm((size_t)2 * nwg), sout(out.size());
        hipLaunchKernelGGL((dev::k_dense_rowstats<DMV_ROWS, DMV_UNR>), dim3(rg, dmv_slices), dim3(dev::TPB), 0, stream,
                           Md, (long long)P.n, (int)P.p, (long long)P.n, (const unsigned char*)offdiag_d.p, spart.p, dmv_qpad, smm.p);
        hipLaunchKernelGGL(dev::k_dense_rowstats_fin, dim3(ceil_div((int)P.p, dev::TPB) + 1), dim3(dev::TPB), 0, stream,
                           (const double*)spart.p, dmv_qpad, dmv_slices, (int)P.p, (const double*)smm.p, nwg, sout.p);
        sout.download(out.data(), out.size(), stream);
        PX_HIP(hipStreamSynchronize(stream));
        st.dense_setup_passes += 1;
    }
    finish_dense_equilibration(P, opt, out.data(), out[(size_t)2 * dmv_qpad], out[(size_t)2 * dmv_qpad + 1]);
    if (!P.equilibrated) return;                         // switched itself off: the plain path, bit for bit
    const double cte = std::sqrt(2.0) / 2.0;
    std::vector<double> dcol(P.n);
    for (int64_t k = 0; k < P.n; ++k) dcol[k] = P.offdiag[k] ? P.Ddiag[k] * cte : P.Ddiag[k];
    drow_d.alloc(std::max<int64_t>(P.p, 1)); dcol_d.alloc(P.n);
    drow_d.upload(P.Ediag.data(), P.p, stream); dcol_d.upload(dcol.data(), P.n, stream);
    PX_HIP(hipStreamSynchronize(stream));
    const double d = P.Ddiag[0];
    dense_frob2 = 0.0;
    for (int64_t i = 0; i < P.p; ++i) dense_frob2 += (P.Ediag[i] * d) * (P.Ediag[i] * d) * out[(size_t)dmv_qpad + i];
}

// sigma_max of the solver's M with a dense A (approx_norm = false, pdhg.jl:108-119): the Lanczos of spectral_norm_host --
// fixed start vector, full re-orthogonalisation, the same stopping rule -- on the SHORT side (M M' when Q <= n: a basis of
// Q-vectors on the host, two passes over the dense block per step).  The products are the loop's own (spmv, dense_mtv).
inline double Solver::spectral_norm_device() {
    const int64_t n = P.n, Q = P.Q;
    if (n == 0 || Q == 0) return 0.0;
    const bool rowside = Q <= n;
    const int64_t dim = rowside ? Q : n;
    const int kmax = (int)std::min<int64_t>(dim, 120);
    DevBuf<double> xd(n), yd(Q), od(rowside ? Q : n);
    std::vector<std::vector<double>> V;
    std::vector<double> al, be, v(dim, 1.0 / std::sqrt((double)dim)), w(dim);
    double sigma2 = 0.0;
    for (int k = 0; k < kmax; ++k) {
        V.push_back(v);
        if (rowside) {                                   // w = M (M' v)
            yd.upload(v.data(), Q, stream);
            dense_mtv(1, yd.p, 0, true, xd.p, 0, nullptr, nullptr, nullptr, 0, false);
            spmv(xd.p, od.p);
        } else {                                         // w = M' (M v)
            xd.upload(v.data(), n, stream);
            spmv(xd.p, yd.p);
            dense_mtv(1, yd.p, 0, true, od.p, 0, nullptr, nullptr, nullptr, 0, false);
        }
        od.download(w.data(), dim, stream);
        PX_HIP(hipStreamSynchronize(stream));
        st.dense_sigma_steps += 1;
        double a = 0.0;
        for (int64_t c = 0; c < dim; ++c) a += w[c] * v[c];
        al.push_back(a);
        for (int pass = 0; pass < 2; ++pass)
            for (const std::vector<double>& vj : V) {
                double h = 0.0;
                for (int64_t c = 0; c < dim; ++c) h += vj[c] * w[c];
                for (int64_t c = 0; c < dim; ++c) w[c] -= h * vj[c];
            }
        double b = 0.0;
        for (int64_t c = 0; c < dim; ++c) b += w[c] * w[c];
        b = std::sqrt(b);
        const int K = k + 1;
        std::vector<double> T((size_t)K * K, 0.0), d(K);
        for (int i = 0; i < K; ++i) { T[(size_t)i * K + i] = al[i]; if (i + 1 < K) T[(size_t)i * K + i + 1] = T[(size_t)(i + 1) * K + i] = be[i]; }
        symeig_dense(K, T.data(), d.data(), true);
        sigma2 = d[K - 1];
        const double resid = std::fabs(b * T[(size_t)(K - 1) * K + (K - 1)]);     // beta * last component of the top Ritz vector
        if (b <= 1e-14 * std::max(1.0, std::fabs(sigma2)) || resid <= 1e-14 * std::fabs(sigma2)) break;
        be.push_back(b);
        for (int64_t c = 0; c < dim; ++c) v[c] = w[c] / b;
    }
    dense_ev_harvest();
    dense_passes_seen = st.dense_passes;                 // (set-up work: not in the iterations' algorithmic bytes)
    return std::sqrt(std::max(sigma2, 0.0));
}

inline void Solver::setup_dense() {
    if (!P.dense()) return;
    upload_dense();
    if (P.equilibrated) {                                // the set-up pass already has the row sums of the scaled block
        g_frob = std::sqrt(dense_frob2 + P.frob * P.frob);
        return;
    }
    // ||M||_F of the column-scaled matrix (pdhg.jl:121 after norm_scaling)
    const int gx = std::min(PSTRIDE, grid_for(P.n));
    hipLaunchKernelGGL(dev::k_dense_frob, dim3(gx), dim3(dev::TPB), 0, stream,
                       Md, (long long)P.n, (int)P.p, (long long)P.n, offdiag_d.p, std::sqrt(2.0) / 2.0, part.p);
    hipLaunchKernelGGL(dev::k_combine_multi, dim3(1), dim3(dev::TPB), 0, stream, (const double*)part.p, PSTRIDE, gx, 0ull, scal.p, 1,
                       (const double*)nullptr, 0, 0, (double*)nullptr);
    double ss = 0.0;
    PX_HIP(hipMemcpyAsync(&ss, scal.p, sizeof(double), hipMemcpyDeviceToHost, stream));
    PX_HIP(hipStreamSynchronize(stream));
    g_frob = std::sqrt(ss + P.frob * P.frob);            // + the sparse rows (G)
}

// every pass over the dense A is bracketed by events (8 ms each at the BASELINE size: the
// bracketing is free); harvested after the iteration's last synchronisation
inline void Solver::dense_ev_begin() {
    if (dense_ev_used == dense_ev.size()) {
        Event a, b;
        a.create(); b.create();
        dense_ev.emplace_back(std::move(a), std::move(b));
    }
    PX_HIP(hipEventRecord(dense_ev[dense_ev_used].first, stream));
}
inline void Solver::dense_ev_end() {
    PX_HIP(hipEventRecord(dense_ev[dense_ev_used].second, stream));
    ++dense_ev_used;
}
inline void Solver::dense_ev_harvest() {
    for (size_t i = 0; i < dense_ev_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, dense_ev[i].first, dense_ev[i].second) == hipSuccess) st.dense_ms += ms;
    }
    dense_ev_used = 0;
}

// y = M (s o x)  (scaled = the solver's M) or M x (the caller's M, exit path)
inline void Solver::dense_mv(const double* x, double* y, bool scaled) {
    if (P.p == 0) return;
    const int rg = ceil_div((int)P.p, DMV_ROWS);
    dense_ev_begin();
    if (scaled && P.equilibrated) {                      // y = E (M (D o s o x))
        hipLaunchKernelGGL((dev::k_dense_mv_eq<DMV_ROWS, DMV_UNR>), dim3(rg, dmv_slices), dim3(dev::TPB), 0, stream,
                           Md, (long long)P.n, (int)P.p, (long long)P.n, x, (const double*)dcol_d.p, dmv_part.p, dmv_qpad);
        hipLaunchKernelGGL(dev::k_dense_mv_fin_eq, dim3(ceil_div((int)P.p, dev::TPB)), dim3(dev::TPB), 0, stream,
                           (const double*)dmv_part.p, dmv_qpad, dmv_slices, (int)P.p, (const double*)drow_d.p, y);
        dense_ev_end();
        st.dense_passes += 1;
        return;
    }
    auto lmv = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(rg, dmv_slices), dim3(dev::TPB), 0, stream,
                           Md, (long long)P.n, (int)P.p, (long long)P.n, x, scaled ? offdiag_d.p : nullptr,
                           std::sqrt(2.0) / 2.0, dmv_part.p, dmv_qpad);
    };
    // shape sweep at n=2000, m=4000 (tools/gpurun_dense_tune.py): <4,4> 6.41, <8,4> 6.55, <4,8> 6.20,
    // <2,8> 6.20, <8,2> 6.51 TB/s
    lmv(dev::k_dense_mv<DMV_ROWS, DMV_UNR>);
    hipLaunchKernelGGL(dev::k_dense_mv_fin, dim3(ceil_div((int)P.p, dev::TPB)), dim3(dev::TPB), 0, stream,
                       dmv_part.p, dmv_qpad, dmv_slices, (int)P.p, y);
    dense_ev_end();
    st.dense_passes += 1;
}

// OUT_c = s o (M' Y_c) [+ addc], c < nc <= 3, one pass over M
inline void Solver::dense_mtv(int nc, const double* Y, long long ystride, bool scaled, double* OUT, long long ostride,
                              const double* old, const double* addc, double* normpart, long long cstride, bool addback) {
    int gx = std::min(PSTRIDE, grid_for(P.n));
    if (gx >= 8) gx &= ~7;                               // multiple of 8: XCD-aware chunk order in the kernel
    const unsigned char* od = scaled ? offdiag_d.p : nullptr;
    const double sc = std::sqrt(2.0) / 2.0;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(gx), dim3(dev::TPB), 0, stream, Md, (long long)P.n, (int)P.p, (long long)P.n,
                           Y, ystride, od, sc, OUT, ostride, old, addc, normpart, cstride,
                           scaled && P.nnz > 0 ? rs.csc_ptr.p : nullptr, rs.csc_row.p, rs.csc_val.p, addback ? 1 : 0);
    };
    auto launch_eq = [&](auto kern) {                    // OUT_c = (D o s) o (M' (E o Y_c)) + the scaled sparse rows
        hipLaunchKernelGGL(kern, dim3(gx), dim3(dev::TPB), 0, stream, Md, (long long)P.n, (int)P.p, (long long)P.n,
                           Y, ystride, (const double*)drow_d.p, (const double*)dcol_d.p, OUT, ostride, old, addc, normpart, cstride,
                           P.nnz > 0 ? rs.csc_ptr.p : nullptr, rs.csc_row.p, rs.csc_val.p, addback ? 1 : 0);
    };
    dense_ev_begin();
    if (scaled && P.equilibrated) {
        if (nc == 1) launch_eq(dev::k_dense_mtv_eq<1, 1, 8>);
        else if (nc == 2) launch_eq(dev::k_dense_mtv_eq<2, 1, 8>);
        else launch_eq(dev::k_dense_mtv_eq<3, 1, 8>);
    }
    else if (nc == 1) launch(dev::k_dense_mtv<1, 1, 8>);
    else if (nc == 2) launch(dev::k_dense_mtv<2, 1, 8>);
    else launch(dev::k_dense_mtv<3, 1, 8>);      // <3,1,16> 6.41, <3,2,8> 6.39, <3,4,4> 6.47, <3,2,4> 6.37 TB/s: flat
    dense_ev_end();
    st.dense_passes += 1;
}

// ---- support-aware path
// S = {i : column i of M is non-empty or c_i != 0}, ascending
inline std::vector<int> Solver::support_list() const {
    std::vector<int> supp;
    for (int64_t k = 0; k < P.n; ++k)
        if (P.colptr[k + 1] > P.colptr[k] || P.c[k] != 0.0) supp.push_back((int)k);
    return supp;
}
// the support's device vectors: the list, its bit mask, c on S, and the buffers k_primal_update_S writes
inline void Solver::upload_support(const std::vector<int>& supp) {
    ns = (int)supp.size();
    supp_h = supp;
    std::vector<unsigned> mask((size_t)(P.n + 31) / 32 + 1, 0u);
    std::vector<double> cS(std::max(ns, 1), 0.0);
    for (int s = 0; s < ns; ++s) { mask[supp[s] >> 5] |= 1u << (supp[s] & 31); cS[s] = P.c[supp[s]]; }
    supp_d.alloc(std::max(ns, 1)); mask_d.alloc(mask.size()); cS_d.alloc(std::max(ns, 1));
    xsave_d.alloc(std::max(ns, 1)); MtyS_cur.alloc(std::max(ns, 1));
    supp_d.upload(supp.data(), ns, stream); mask_d.upload(mask.data(), mask.size(), stream);
    cS_d.upload(cS.data(), ns, stream);
    MtyS_cur.zero(stream); xsave_d.zero(stream);
    esv_d.alloc((size_t)2 * std::max(ns, 1)); esv_d.zero(stream);
    PX_HIP(hipStreamSynchronize(stream));                 // host vectors go out of scope
}
// does a model whose support list has `ns` entries run the support path (the options, the cones, the auto rule)
inline bool Solver::support_path_wanted(size_t ns) const {
    // (without linesearch the support path runs on request -- support_path = 1 -- and inside a block-sharded solve, which is built on it)
    if (opt.support_path == 0 || (!opt.line_search_flag && opt.support_path < 0)) return false;
    if (!P.socs.empty() || !one_blocks.empty() || P.blocks.empty()) return false;
    if (opt.support_path < 0 && (8 * (int64_t)ns > P.n || P.n < 4096)) return false;   // auto: only when it pays
    return true;
}
// One PSD block's share of setup_support: the support entries supp[s0 .. s1) that lie in block B as a symmetric sparse matrix in
// ELL form (at most 32 entries a row, the rest of a hub row in the overflow list), and the operator form's workspaces.  W.fop_ok
// says whether the block takes the operator form (not with hub rows under the auto rule below).  The entries' indices into the
// support-value array are those of the whole list.
inline void Solver::build_block_operator(EigWork& W, const BlockInfo& B, const std::vector<int>& supp, size_t s0, size_t s1) {
    std::vector<int> cnt(W.npad, 0);
    std::vector<std::array<int, 3>> ent;                 // row, col, s
    ent.reserve(2 * (s1 - s0));
    for (size_t sidx = s0; sidx < s1; ++sidx) {
        const int64_t k = supp[sidx] - B.off;
        int64_t j = (int64_t)((std::sqrt(8.0 * (double)k + 1.0) - 1.0) / 2.0);
        while ((j + 1) * (j + 2) / 2 <= k) ++j;
        while (j * (j + 1) / 2 > k) --j;
        const int i = (int)(k - j * (j + 1) / 2);
        ent.push_back({i, (int)j, (int)sidx}); cnt[i]++;
        if (i != (int)j) { ent.push_back({(int)j, i, (int)sidx}); cnt[j]++; }
    }
    int wmax = 1;
    for (int c : cnt) wmax = std::max(wmax, c);
    // ELL part of at most 32 entries per row; the rest of a wider (hub) row goes to an
    // overflow list that the row's workgroup reduces cooperatively
    const int w = std::min(wmax, 32);
    // measured (tools/gpurun_opcmp.py): below n ~ 2000 the two operators cost the same
    // (latency-bound), and a hub row costs the operator form ~15 us per mat-vec at
    // n = 1000 (maxG51) -- more than streaming a packed triangle of up to ~100 MB.  With
    // hub rows the operator form is therefore only taken for large blocks.
    if (wmax > w && B.n < 6000 && opt.lanczos_operator < 0) return;
    std::vector<int> col((size_t)w * W.npad), sx((size_t)w * W.npad, -1);
    for (int k = 0; k < w; ++k) for (int i = 0; i < W.npad; ++i) col[(size_t)k * W.npad + i] = i;
    std::vector<std::vector<std::array<int, 2>>> over(W.npad);
    std::fill(cnt.begin(), cnt.end(), 0);
    for (const auto& e : ent) {
        const int kk = cnt[e[0]]++;
        if (kk < w) { const size_t at = (size_t)kk * W.npad + e[0]; col[at] = e[1]; sx[at] = e[2]; }
        else over[e[0]].push_back({e[1], e[2]});
    }
    W.ell_w = w;
    W.ell_col.alloc(col.size()); W.ell_sidx.alloc(sx.size());
    W.ell_col.upload(col.data(), col.size(), stream); W.ell_sidx.upload(sx.data(), sx.size(), stream);
    W.ov = dev::EllOverflow{};
    if (wmax > w) {
        std::vector<int> wptr(W.nt + 1, 0), wrow, wlo, whi, ocol, osx;
        for (int g = 0; g < W.nt; ++g) {
            for (int rl = 0; rl < dev::LZ_ROWS; ++rl) {
                const int row = g * dev::LZ_ROWS + rl;
                if (row >= W.npad || over[row].empty()) continue;
                wrow.push_back(rl); wlo.push_back((int)ocol.size());
                for (const auto& e : over[row]) { ocol.push_back(e[0]); osx.push_back(e[1]); }
                whi.push_back((int)ocol.size());
            }
            wptr[g + 1] = (int)wrow.size();
        }
        W.wr_ptr.alloc(wptr.size()); W.wr_row.alloc(wrow.size()); W.wr_lo.alloc(wlo.size()); W.wr_hi.alloc(whi.size());
        W.ov_col.alloc(ocol.size()); W.ov_sidx.alloc(osx.size());
        W.wr_ptr.upload(wptr.data(), wptr.size(), stream); W.wr_row.upload(wrow.data(), wrow.size(), stream);
        W.wr_lo.upload(wlo.data(), wlo.size(), stream); W.wr_hi.upload(whi.data(), whi.size(), stream);
        W.ov_col.upload(ocol.data(), ocol.size(), stream); W.ov_sidx.upload(osx.data(), osx.size(), stream);
        W.ov = dev::EllOverflow{W.wr_ptr.p, W.wr_row.p, W.wr_lo.p, W.wr_hi.p, W.ov_col.p, W.ov_sidx.p};
        PX_HIP(hipStreamSynchronize(stream));             // host vectors go out of scope
    }
    W.F.alloc((size_t)W.npad * W.cap); W.F.zero(stream);
    W.Flam.alloc(std::max(W.n, dev::MAXK)); W.Flam.zero(stream);
    W.tpart.alloc((size_t)dev::MAXK * W.pld); W.tpart.zero(stream);
    W.tred.alloc(dev::RLD); W.tred.zero(stream);
    W.ebuf.alloc(W.npad); W.ebuf.zero(stream);
    W.apartf.alloc(W.pld); W.apartf.zero(stream);
    W.warm_part.alloc(ceil_div(W.npad, dev::TPB)); W.warm_part.zero(stream);
    PX_HIP(hipStreamSynchronize(stream));                 // host vectors go out of scope
    W.fop_ok = true;
}
inline void Solver::setup_support() {
    use_support = false;
    const std::vector<int> supp = support_list();
    if (!support_path_wanted(supp.size())) return;
    upload_support(supp);
    // residual partial slots: one per reconstruction tile of every block + the tail workgroups
    tile_base.clear();
    int base = 0;
    for (const BlockInfo& B : P.blocks) {
        tile_base.push_back(base);
        const int nt = ceil_div(B.n, dev::TILE);
        base += tile_grid(nt);                           // reconstruction grid
    }
    tile_base.push_back(base);
    if (P.sdplen < P.n) base += std::min(256, ceil_div(P.n - P.sdplen, dev::TPB));
    n_res_wg = base;
    rstride = base;
    respart_d.alloc((size_t)2 * std::max(base, 1)); respart_d.zero(stream);
    // operator-form mat-vec: the support update as a symmetric sparse matrix per block (ELL)
    if (opt.lanczos_operator != 0) {
        size_t s0 = 0;
        for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
            const BlockInfo& B = P.blocks[idx];
            EigWork& W = eig[idx];
            size_t s1 = s0;
            while (s1 < supp.size() && supp[s1] < B.off + B.N) ++s1;     // supp is ascending
            if (B.n < 2 || W.npad == 0) { s0 = s1; continue; }
            build_block_operator(W, B, supp, s0, s1);
            s0 = s1;
        }
    }
    PX_HIP(hipStreamSynchronize(stream));
    use_support = true;
}

// sparse operator on the device, both orientations, int32 indices
inline void Solver::upload_sparse_operator() {
    build_rows();
    rs.csr_val.upload(P.rval.data(), P.nnz, stream); rs.csc_val.upload(P.val.data(), P.nnz, stream);
    upload_pattern(rs, P);
}
// The pattern of R's operator into `to`: pointers and indices in both orientations, the position maps where `to` has them, and
// what M x derives from the row pointers -- a wave per row above 8 entries a row on average, the segments of the long rows.
// R: the solver's Prep, or the one a row change is about to commit (the next row state is built before it is the solver's).
inline void Solver::upload_pattern(RowState& to, const Prep& R) {
    std::vector<int> rp(R.Q + 1), cp(R.n + 1);
    // (prepare() and plan_rows() guarantee n, Q, nnz < 2^31: the casts below cannot truncate)
    for (int64_t i = 0; i <= R.Q; ++i) rp[i] = (int)R.rowptr[i];
    for (int64_t i = 0; i <= R.n; ++i) cp[i] = (int)R.colptr[i];
    to.csr_ptr.upload(rp.data(), R.Q + 1, stream); to.csc_ptr.upload(cp.data(), R.n + 1, stream);
    to.csr_col.upload(R.colidx.data(), R.nnz, stream); to.csc_row.upload(R.rowidx.data(), R.nnz, stream);
    if (to.csc_pos_d.n > 0) { to.csc_pos_d.upload(R.csc_pos.data(), R.nnz, stream); to.csr_pos_d.upload(R.csr_pos.data(), R.nnz, stream); }
    PX_HIP(hipStreamSynchronize(stream));
    to.csr_wave = R.Q > 0 && (double)R.nnz / (double)R.Q > 8.0;
    setup_long_rows(to, rp);
}

// ---- state seam (include/proxsdp_hip.h proxsdp_state)
inline void Solver::check_state_shape(const proxsdp_state& s, const char* what) const {
    const std::string w(what);
    if (s.struct_size != (int64_t)sizeof(proxsdp_state)) throw std::invalid_argument(w + " state: struct_size mismatch");
    if (s.n != P.n || s.Q != P.Q || s.n_psd != (int64_t)P.blocks.size())
        throw std::invalid_argument(w + " state: n / Q / n_psd do not match the problem");
    if (s.hist_len != 2 * (int64_t)opt.convergence_window)
        throw std::invalid_argument(w + " state: hist_len must be 2 * convergence_window");
    if (s.iteration < 1) throw std::invalid_argument(w + " state: iteration must be >= 1");
    if (!s.x || !s.Mty || !s.hist || (P.Q > 0 && (!s.y || !s.Mx)) ||
        (!P.blocks.empty() && (!s.target_rank || !s.current_rank || !s.min_eig)))
        throw std::invalid_argument(w + " state: NULL array");
    if (sharded() || P.equilibrated) throw std::domain_error("state capture / resume: not with a block-sharded solve or equilibration");
}

// continue from req.resume_state: called after the "Init" section built every buffer; overwrites the initial point
inline void Solver::apply_resume() {
    const proxsdp_state& s = *req.resume_state;
    check_state_shape(s, "resume");
    xbuf[xc].upload(s.x, P.n, stream);
    rs.ybuf[yc].upload(s.y, P.Q, stream);
    rs.Mxbuf[mxc].upload(s.Mx, P.Q, stream);
    Mtybuf[mtyc].upload(s.Mty, P.n, stream);
    std::vector<double> mtyS;
    if (use_support) {                                   // the support path carries M'y on the support only
        std::vector<int> supp(ns);
        supp_d.download(supp.data(), ns, stream);
        PX_HIP(hipStreamSynchronize(stream));
        mtyS.resize(std::max(ns, 1), 0.0);
        for (int q = 0; q < ns; ++q) mtyS[q] = s.Mty[supp[q]];
        MtyS_cur.upload(mtyS.data(), ns, stream);
    }
    PX_HIP(hipStreamSynchronize(stream));
    primal_step = s.scal[0]; primal_step_old = s.scal[1]; dual_step = s.scal[2];
    beta = s.scal[3]; theta = s.scal[4]; adapt_level = s.scal[5];
    equa_feasibility = s.scal[6]; ineq_feasibility = s.scal[7]; dual_feasibility = s.scal[8];
    rank_update = (int)s.ints[0]; update_cont = (int)s.ints[1]; ada_count = (int)s.ints[2];
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
        target_rank[idx] = std::min<long long>(std::max<long long>(s.target_rank[idx], 1), P.blocks[idx].n);
        current_rank[idx] = s.current_rank[idx];
        min_eig[idx] = s.min_eig[idx];
    }
    CircularVector* H[PROXSDP_STATE_NHIST] = {&h_gap, &h_pobj, &h_dobj, &h_feas, &h_pres, &h_dres, &h_comb};
    for (int q = 0; q < PROXSDP_STATE_NHIST; ++q)
        std::copy(s.hist + (size_t)q * s.hist_len, s.hist + (size_t)(q + 1) * s.hist_len, H[q]->v.begin());
    iter = s.iteration;
    // the iterate is a general matrix now: neither zero off the support nor known in factored form
    for (EigWork& W : eig) { W.have_factors = false; W.xprev.sparse = false; }
}

// enter the loop from the caller's point (include/proxsdp_hip.h proxsdp_start; validated by the entry point): called after
// the "Init" section built every buffer and the cold point.  Nothing of size n is built in a host loop: the point is uploaded
// as the caller holds it and brought into the solver's order and scale by k_start_gather; a factored cone goes through the
// solver's own reconstruction launch straight into the iterate; M x and M'y come from the solver's product launches.
inline void Solver::apply_start() {
    const proxsdp_start& s = *req.start_point();
    const size_t nb = P.blocks.size();
    auto given = [&](size_t idx) -> long long { return s.n_psd > 0 ? (long long)s.rank[idx] : -1; };
    // target ranks and step scalars: they hold for a start without a point as well
    bool any_fac = false;
    for (size_t idx = 0; idx < nb; ++idx) {
        const long long side = P.blocks[idx].n, r = given(idx);
        any_fac = any_fac || r >= 0;
        if (s.target_rank && s.target_rank[idx] > 0) target_rank[idx] = std::min<long long>(s.target_rank[idx], side);
        else if (r >= 0) target_rank[idx] = std::min<long long>(side, std::max<long long>(std::max(opt.initial_target_rank, 1), r + 1));
    }
    if (s.primal_step > 0.0) { primal_step = s.primal_step; primal_step_old = primal_step; dual_step = primal_step; }
    if (s.beta > 0.0) beta = s.beta;
    // vectors the caller holds on the device (proxsdp_hip_solve_device): read where they are
    const proxsdp_device_vectors* sd = req.start_dev;
    const double* d_primal = sd ? sd->primal : nullptr;
    const double* d_eq = sd ? sd->dual_eq : nullptr;
    const double* d_in = sd ? sd->dual_in : nullptr;
    if (sd) check_start_dev();
    // no point given: the cold vectors stay (x_old = 0)
    if (!s.primal && !s.dual_eq && !s.dual_in && !d_primal && !d_eq && !d_in && !any_fac) return;
    start_active = true;
    if (P.equilibrated && Ddiag_d.n == 0) {                              // (the exit path finds them uploaded)
        Ddiag_d.alloc(P.n); Ediag_d.alloc(std::max<int64_t>(P.Q, 1));
        Ddiag_d.upload(P.Ddiag.data(), P.n, stream); Ediag_d.upload(P.Ediag.data(), P.Q, stream);
    }
    const double sqrt2 = std::sqrt(2.0);
    start_src_d.alloc((size_t)std::max<int64_t>(std::max(P.n, P.Q), 1));
    auto gather = [&](const double* src, long long s0, const long long* ord, const unsigned char* od, const double* D,
                      double* out, long long k0, long long k1) {
        if (k1 <= k0) return;
        hipLaunchKernelGGL(dev::k_start_gather, dim3(grid_for(k1 - k0)), dim3(dev::TPB), 0, stream,
                           src, s0, ord, od, D, sqrt2, out, k0, k1);
    };
    if (s.primal || d_primal) {                          // every entry outside the factored cones
        static_assert(sizeof(long long) == sizeof(int64_t), "variable order is uploaded as it is");
        if (start_ord_d.n != (size_t)P.n) {               // (a model handle's later solves find it uploaded)
            start_ord_d.alloc(P.n);
            start_ord_d.upload(reinterpret_cast<const long long*>(P.ord.data()), P.n, stream);
        }
        if (offdiag_d.n == 0) { offdiag_d.alloc(P.n); offdiag_d.upload(P.offdiag.data(), P.n, stream); }
        const double* src = d_primal;
        if (!src) { start_src_d.upload(s.primal, P.n, stream); src = start_src_d.p; }
        const double* Dd = P.equilibrated ? Ddiag_d.p : nullptr;
        long long k = 0;
        for (size_t idx = 0; idx < nb; ++idx) {
            if (given(idx) < 0) continue;
            gather(src, 0, start_ord_d.p, offdiag_d.p, Dd, xbuf[xc].p, k, P.blocks[idx].off);
            k = P.blocks[idx].off + P.blocks[idx].N;
        }
        gather(src, 0, start_ord_d.p, offdiag_d.p, Dd, xbuf[xc].p, k, P.n);
        PX_HIP(hipGetLastError());
        PX_HIP(hipStreamSynchronize(stream));            // (start_src_d takes the duals next)
    }
    std::vector<double> ones(nb, 0.0), lamh;
    for (size_t idx = 0; idx < nb; ++idx) {              // factored cones: x_k = V diag(lambda / d) V' (D = d I)
        const long long r = given(idx);
        if (r < 0) continue;
        const BlockInfo& B = P.blocks[idx];
        double* xp = xbuf[xc].p + B.off;
        if (r == 0) { PX_HIP(hipMemsetAsync(xp, 0, (size_t)B.N * sizeof(double), stream)); continue; }
        const double* V = s.vectors + s.vec_ptr[idx];
        const double* lam = s.values + s.val_ptr[idx];
        lamh.assign(lam, lam + r);
        if (P.equilibrated) for (double& v : lamh) v /= P.Ddiag[B.off];
        if (B.n == 1) {                                  // (no workspace: the one entry, in the kernel's order of operations)
            ones[idx] = V[0] * (V[0] * lamh[0]);
            PX_HIP(hipMemcpyAsync(xp, &ones[idx], sizeof(double), hipMemcpyHostToDevice, stream));
            continue;
        }
        EigWork& W = eig[idx];
        start_V.alloc((size_t)W.npad * r); start_V.zero(stream);       // padded to the workspace's leading dimension
        PX_HIP(hipMemcpy2DAsync(start_V.p, (size_t)W.npad * sizeof(double), V, (size_t)B.n * sizeof(double),
                                (size_t)B.n * sizeof(double), (size_t)r, hipMemcpyHostToDevice, stream));
        start_lam.alloc(r); start_lam.upload(lamh.data(), r, stream);
        launch_reconstruct(W, start_V.p, W.npad, start_lam.p, (int)r, xp);
        PX_HIP(hipGetLastError());
        PX_HIP(hipStreamSynchronize(stream));            // (the staging buffers serve the next cone)
    }
    if (P.Q > 0 && (s.dual_eq || s.dual_in || d_eq || d_in)) {   // y = [dual_eq; dual_in] / E, then M'y
        // a half given on the host, or not at all, is staged in start_src_d; one on the device is read where it is
        if (s.dual_eq) start_src_d.upload(s.dual_eq, P.p, stream);
        else if (!d_eq && P.p > 0) PX_HIP(hipMemsetAsync(start_src_d.p, 0, (size_t)P.p * sizeof(double), stream));
        if (s.dual_in) PX_HIP(hipMemcpyAsync(start_src_d.p + P.p, s.dual_in, (size_t)P.m * sizeof(double), hipMemcpyHostToDevice, stream));
        else if (!d_in && P.m > 0) PX_HIP(hipMemsetAsync(start_src_d.p + P.p, 0, (size_t)P.m * sizeof(double), stream));
        const double* Ed = P.equilibrated ? Ediag_d.p : nullptr;
        if (!d_eq && !d_in) {
            gather(start_src_d.p, 0, nullptr, nullptr, Ed, rs.ybuf[yc].p, 0, P.Q);
        } else {
            gather(d_eq ? d_eq : start_src_d.p, 0, nullptr, nullptr, Ed, rs.ybuf[yc].p, 0, P.p);
            gather(d_in ? d_in : start_src_d.p, d_in ? P.p : 0, nullptr, nullptr, Ed, rs.ybuf[yc].p, P.p, P.Q);
        }
        const BatchShape b = batch_shape();
        PX_HIP(hipMemcpyAsync(rs.ycand_d.p, rs.ybuf[yc].p, (size_t)P.Q * sizeof(double), hipMemcpyDeviceToDevice, stream));
        dev::TrialBatch tb{};                            // ONE plain candidate: M'y as computed (on the support, or every column)
        tb.nc = 1; tb.plain = 1;
        batch_mty(tb, 1);
        PX_HIP(hipMemcpyAsync(b.mty_cur, Mtycand_d.p, (size_t)b.cnt * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    spmv(xbuf[xc].p, rs.Mxbuf[mxc].p);                      // M x (sparse rows, and the dense block with its scale vectors)
    PX_HIP(hipGetLastError());
    PX_HIP(hipStreamSynchronize(stream));
    if (P.dense()) { dense_ev_harvest(); dense_passes_seen = st.dense_passes; }   // (set-up work, as the sigma_max passes)
    // the ping-pong pairs' current buffers hold the point, so x_old = x, y_old = y, (M x)_old = M x, (M'y)_old = M'y at
    // iteration 1; the iterate is a general matrix: the first projection reads the packed buffer
    for (EigWork& W : eig) { W.have_factors = false; W.xprev.sparse = false; W.ritz_ok = false; }
}

// proxsdp_hip_start_point: the internal vectors after the start path
inline void Solver::write_start_point() {
    proxsdp_state& s = *req.start_out;
    PX_HIP(hipStreamSynchronize(stream));
    xbuf[xc].download(s.x, P.n, stream);
    if (P.Q > 0) { rs.ybuf[yc].download(s.y, P.Q, stream); rs.Mxbuf[mxc].download(s.Mx, P.Q, stream); }
    if (use_support) {
        std::vector<int> supp(ns);
        std::vector<double> mtyS(std::max(ns, 1), 0.0);
        supp_d.download(supp.data(), ns, stream);
        MtyS_cur.download(mtyS.data(), ns, stream);
        PX_HIP(hipStreamSynchronize(stream));
        std::fill(s.Mty, s.Mty + P.n, 0.0);
        for (int q = 0; q < ns; ++q) s.Mty[supp[q]] = mtyS[q];
    } else {
        Mtybuf[mtyc].download(s.Mty, P.n, stream);
    }
    PX_HIP(hipStreamSynchronize(stream));
    s.scal[0] = primal_step; s.scal[1] = primal_step_old; s.scal[2] = dual_step;
    s.scal[3] = beta; s.scal[4] = theta; s.scal[5] = adapt_level;
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) s.target_rank[idx] = target_rank[idx];
    s.iteration = 0;
}

// write req.capture_state: the stream is idle (every iteration ends with a synchronisation)
inline void Solver::write_capture() {
    proxsdp_state& s = *req.capture_state;
    if (certificate_search) return;          // (the seam does not carry a certificate search: ints[3] stays 0, the solve goes on)
    PX_HIP(hipStreamSynchronize(stream));
    harvest_small_ranks();
    xbuf[xc].download(s.x, P.n, stream);
    rs.ybuf[yc].download(s.y, P.Q, stream);
    rs.Mxbuf[mxc].download(s.Mx, P.Q, stream);
    if (use_support) {
        std::vector<int> supp(ns);
        std::vector<double> mtyS(std::max(ns, 1), 0.0);
        supp_d.download(supp.data(), ns, stream);
        MtyS_cur.download(mtyS.data(), ns, stream);
        PX_HIP(hipStreamSynchronize(stream));
        std::fill(s.Mty, s.Mty + P.n, 0.0);
        for (int q = 0; q < ns; ++q) s.Mty[supp[q]] = mtyS[q];
    } else {
        Mtybuf[mtyc].download(s.Mty, P.n, stream);
    }
    PX_HIP(hipStreamSynchronize(stream));
    std::fill(std::begin(s.scal), std::end(s.scal), 0.0);
    std::fill(std::begin(s.ints), std::end(s.ints), 0);
    s.scal[0] = primal_step; s.scal[1] = primal_step_old; s.scal[2] = dual_step;
    s.scal[3] = beta; s.scal[4] = theta; s.scal[5] = adapt_level;
    s.scal[6] = equa_feasibility; s.scal[7] = ineq_feasibility; s.scal[8] = dual_feasibility;
    s.ints[0] = rank_update; s.ints[1] = update_cont; s.ints[2] = ada_count;
    for (size_t idx = 0; idx < P.blocks.size(); ++idx) {
        s.target_rank[idx] = target_rank[idx]; s.current_rank[idx] = current_rank[idx]; s.min_eig[idx] = min_eig[idx];
    }
    CircularVector* H[PROXSDP_STATE_NHIST] = {&h_gap, &h_pobj, &h_dobj, &h_feas, &h_pres, &h_dres, &h_comb};
    for (int q = 0; q < PROXSDP_STATE_NHIST; ++q) std::copy(H[q]->v.begin(), H[q]->v.end(), s.hist + (size_t)q * s.hist_len);
    s.ints[3] = 1;
}

// ------------------------------------------------------------------ chambolle_pock (pdhg.jl:1-530) in phases
inline void Solver::check_run_options() {
    if (sharded()) reject_for_shard(false, !opt.approx_norm, false);
    if (P.n <= 0) throw std::invalid_argument("problem has no variables");
    if (opt.convergence_window <= 0) throw std::invalid_argument("convergence_window must be positive");
    // (the reference's `for i in 1:max_linsearch_steps` simply runs no trial then and keeps stale norms; the batched
    // candidates here need at least one)
    if (opt.line_search_flag && opt.max_linsearch_steps < 1) throw std::invalid_argument("max_linsearch_steps must be >= 1");
    // fault injection is a TEST switch: it only works in a process that asks for it by environment as well
    if (opt.debug_fail_iteration > 0) {
        const char* e = std::getenv("PROXSDP_HIP_FAULT_INJECTION");
        if (!(e && e[0] == '1')) throw std::invalid_argument("debug_fail_iteration needs PROXSDP_HIP_FAULT_INJECTION=1 in the environment (test switch)");
    }
}

// Params and Residuals of the reference at their initial values (host state only)
inline void Solver::init_parameters() {
    theta = opt.initial_theta; adapt_level = opt.initial_adapt_level; beta = opt.initial_beta;
    const int window = opt.convergence_window;
    const size_t nb = P.blocks.size();
    target_rank.assign(nb, 2); current_rank.assign(nb, 2); min_eig.assign(nb, 0.0);
    for (size_t idx = 0; idx < nb; ++idx)               // 2 in the reference (pdhg.jl:19-20)
        target_rank[idx] = std::min<long long>(std::max(opt.initial_target_rank, 1), P.blocks[idx].n);
    time_limit = opt.time_limit;
    ada_count = 0;
    h_gap.init(2 * window); h_pobj.init(2 * window); h_dobj.init(2 * window); h_feas.init(2 * window);
    h_pres.init(2 * window); h_dres.init(2 * window); h_comb.init(2 * window);
}

// global constants (sums over shards of a block-sharded solve; local values otherwise), and the iteration limit they choose
inline void Solver::reduce_global_constants() {
    double pw = (double)P.p, mw = (double)P.m, nb2 = P.norm_b * P.norm_b, nh2 = P.norm_h * P.norm_h;
    for (size_t k = 0; k < coup_rows.size(); ++k) {          // a coupling row counts on its owner only
        if (coup_owned[k]) continue;
        const int r = coup_rows[k];
        if (r < P.p) { pw -= 1.0; nb2 -= P.b_orig[r] * P.b_orig[r]; }
        else { mw -= 1.0; nh2 -= P.h_orig[r - P.p] * P.h_orig[r - P.p]; }
    }
    std::vector<double> sums = {(double)P.n, pw, mw, std::max(nb2, 0.0), std::max(nh2, 0.0),
                                P.norm_c * P.norm_c, P.frob * P.frob};
    std::vector<double> maxs = {(!P.blocks.empty() || !P.socs.empty()) ? 1.0 : 0.0};
    reduce(sums, maxs);
    g_n = sums[0]; g_p = sums[1]; g_m = sums[2]; g_Q = g_p + g_m;
    g_norm_b = sharded() ? std::sqrt(sums[3]) : P.norm_b;
    g_norm_h = sharded() ? std::sqrt(sums[4]) : P.norm_h;
    g_norm_c = sharded() ? std::sqrt(sums[5]) : P.norm_c;
    g_frob = sharded() ? std::sqrt(sums[6]) : P.frob;
    g_conic = maxs[0] > 0.5;
    // (a block-sharded solve chooses its vector path per shard: the library-only knob support_path is overridden in
    //  classify_blocks; check_dual_feas and line_search_flag = false are served on both)
    if (opt.max_iter <= 0) max_iter_local = g_conic ? opt.max_iter_conic : opt.max_iter_lp;
    else max_iter_local = opt.max_iter;
}

// the threads that help from the host side: rocSOLVER's loader (opt-in) and the QL helpers
inline void Solver::start_host_helpers() {
    bool big_block = false;
    for (const BlockInfo& B : P.blocks) big_block = big_block || B.n >= 256;
    // opt-in only: measured on MI355X/ROCm 7.2, loading rocSOLVER's code objects from a second
    // thread stalls this thread's kernel launches (a 0.3 s solve took 8 s), so by default the
    // exit path pays the one-off ~3 s initialisation itself in a cold process
    if (big_block && opt.rocsolver_warmup == 1) start_rocsolver_warmup();
    if (opt.host_eig_threads > 0) QlPool::get().ensure(opt.host_eig_threads);
}

// the four ping-pong pairs of the iterate, zero (also what the kernel-level test entries start from: they upload their own
// c and [b; h], so the rest of alloc_iterate is not theirs)
inline void Solver::alloc_iterate_pairs() {
    build_rows();
    for (int k = 0; k < 2; ++k) {
        xbuf[k].alloc(P.n); Mtybuf[k].alloc(P.n);
        xbuf[k].zero(stream); Mtybuf[k].zero(stream); rs.ybuf[k].zero(stream); rs.Mxbuf[k].zero(stream);
    }
    xc = yc = mxc = mtyc = 0;
}

// x, y, M x, M'y; c and [b; h]; the coupling rows of a block-sharded solve; the reduction scratch
inline void Solver::alloc_iterate() {
    alloc_iterate_pairs();
    c_d.alloc(P.n); c_d.upload(P.c.data(), P.n, stream);
    {
        const std::vector<double> bh = stacked_bh(P.b, P.h);
        rs.bh_d.upload(bh.data(), P.Q, stream);
        PX_HIP(hipStreamSynchronize(stream));
    }
    if (!coup_rows.empty()) {
        coup_rows_d.alloc(coup_rows.size()); roww_d.alloc(std::max<int64_t>(P.Q, 1));
        std::vector<double> rw(P.Q, 1.0);
        for (size_t k = 0; k < coup_rows.size(); ++k) if (!coup_owned[k]) rw[coup_rows[k]] = 0.0;
        coup_rows_d.upload(coup_rows.data(), coup_rows.size(), stream);
        roww_d.upload(rw.data(), P.Q, stream);
        PX_HIP(hipStreamSynchronize(stream));
        comm->setup_coupling(coup_rows.size(), stream);
    }
    part.alloc((size_t)NQ * PSTRIDE); part.zero(stream);
    scal.alloc(NQ); scal.zero(stream);
}

// the PSD blocks by the engine that projects them -- 1x1 (clamped), small (one batched launch), large (an eigensolver each)
// -- with every eigensolver block's Lanczos workspace and start vector; a shard's vector path
inline void Solver::classify_blocks() {
    const size_t nb = P.blocks.size();
    eig.resize(nb);
    // small blocks by the sign function in one launch: auto (and small_block_batch = 2) unless the tiled sign projection is
    // switched off or the solve asks for tolerances below that engine's 1e-10-of-the-scale floor (as full_eig_by_sign)
    const bool small_sign = opt.small_block_batch == 2 ||
        (opt.small_block_batch < 0 && opt.full_eig_sign != 0 &&
         std::min({opt.tol_gap, opt.tol_feasibility, opt.tol_primal, opt.tol_dual}) >= 1e-8);
    small_jacobi_max = small_sign ? (opt.small_block_batch == 2 ? 1 : 2) : 64;   // (measured, tools/gpurun_jacobi_vs_sign.py: from side 3 on the sign kernel wins)
    // block-sharded solve: the vector path of THIS shard, known before the block lists are built.  A shard whose cones allow
    // the support path (at least one PSD block, no SOC, no 1x1 block -- setup_support's own conditions) runs it, as every
    // sharded solve used to, with its small blocks not batched; any other shard runs the general path with the small-block
    // launches of a single-process solve.  Shards of one solve may differ: only reduced scalars steer the iteration.
    shard_general = false;
    if (sharded()) {
        shard_general = P.blocks.empty() || !P.socs.empty();
        for (const BlockInfo& B : P.blocks) shard_general = shard_general || B.n == 1;
        opt.support_path = shard_general ? 0 : 1;
        general_row_weights = shard_general;
    }
    const double* ur = user_resid;
    for (size_t idx = 0; idx < nb; ++idx) {
        const BlockInfo& B = P.blocks[idx];
        if (B.n == 1) { one_blocks.push_back((int)idx); if (ur) ur += 1; continue; }
        EigWork& W = eig[idx];
        big_blocks.push_back((int)idx);
        // side 2..64 and never on the Krylov path: ONE launch for all of them (dense vector path): batched Jacobi
        // (auto: side 2 only -- measured: 80 / 140 / 370 us per iteration at side 3 / 8 / 16 where the sign kernel stays at 60; at side 22 the
        // single-workgroup Jacobi takes 950 us, at side 50 5.9 ms against
        // 1.1 ms for one rocSOLVER call; two blocks of side 10 and 5: 1.4x faster batched; seven of side 2: 6.4x) and,
        // round 5, the one-workgroup LDS-resident sign projection (small_sign.hip.hpp) for sides 3 .. 64
        if (opt.small_block_batch != 0 && B.n <= (small_sign ? std::max(small_jacobi_max, std::min(64, small_sign_cap)) : (opt.small_block_batch > 0 ? 64 : 32)) &&
            B.n <= opt.min_size_krylov_eigs && (!sharded() || shard_general))
            small_blocks.push_back((int)idx);
        else
            large_blocks.push_back((int)idx);
        // Krylov workspace: the largest target rank the Krylov path may see, and room for
        // full_eig!-by-Lanczos (up to 94 pairs) on blocks that can take it
        int max_nev = std::min<int>(std::max<int>(opt.max_target_rank_krylov_eigs, 2), B.n);
        if (opt.full_eig_lanczos != 0 && B.n > opt.min_size_krylov_eigs && B.n >= 400)
            max_nev = std::max(max_nev, std::min(94, B.n / 4));
        alloc_eigwork(W, B.n, max_nev);
        lanczos_start_vector(W, ur);
        if (ur) ur += B.n;
        W.resid.upload(W.resid_host.data(), W.npad, stream);
    }
    if (small_blocks.size() < 2 && opt.small_block_batch < 0 && !small_sign) {   // auto, Jacobi only: a batch needs several blocks
        large_blocks = big_blocks; small_blocks.clear();
    }
}

// several eigensolver-sized blocks: project them concurrently, one worker thread and one
// stream per block (the per-block Lanczos chains are launch-latency-bound, so they overlap
// almost perfectly: MIMO n=512 x 8 on one GPU).  options.block_threads = 0 disables.
inline void Solver::start_block_workers() {
    if (block_pool) return;                              // (a model handle calls this before every solve)
    int nthreads = opt.block_threads < 0 ? 8 : std::min(opt.block_threads, 64);
    // (blocks handled by the batched small-block kernel need no worker / stream of their own)
    const std::vector<int>& pool_blocks = small_blocks.empty() ? big_blocks : large_blocks;
    nthreads = std::min<int>(nthreads, (int)pool_blocks.size());
    if (nthreads < 2) return;
    for (int idx : pool_blocks) {
        eig[idx].stream.create();
        eig[idx].done.create(hipEventDisableTiming);
    }
    ev_main.create(hipEventDisableTiming);
    PX_HIP(hipStreamSynchronize(stream));           // workspace zero-fills precede any block-stream work
    const int dev_id = opt.device_id;
    std::atomic<long long>* const sink = DevAccount::sink;
    block_pool.reset(new BlockPool(nthreads, [dev_id, sink]() { (void)hipSetDevice(dev_id); DevAccount::sink = sink; }));
}

// the batched small-block launch: offsets, sides and rank records of its blocks, and the kernels' LDS grants
inline void Solver::setup_small_batch() {
    if (small_blocks.empty()) return;
    std::vector<long long> so; std::vector<int> ss;
    for (int idx : small_blocks) { so.push_back(P.blocks[idx].off); ss.push_back(P.blocks[idx].n); small_maxn = std::max(small_maxn, P.blocks[idx].n); }
    small_off.alloc(so.size()); small_side.alloc(ss.size()); small_rank.alloc(4 * ss.size() + 2); small_rank.zero(stream);   // [rank | npos | schedule-test outcome | Jacobi sweeps] per block
    small_off.upload(so.data(), so.size(), stream); small_side.upload(ss.data(), ss.size(), stream);
    small_rank_host.alloc(2 * ss.size() + 2);      // (ints, two per slot: rank | positive count | schedule-test outcome | Jacobi sweeps per block)
    small_sign_maxn = 0;
    int jac_maxn = 0;
    for (int sd : ss) { if (sd > small_jacobi_max) small_sign_maxn = std::max(small_sign_maxn, sd); else jac_maxn = std::max(jac_maxn, sd); }
    const size_t lds = ((size_t)2 * jac_maxn * (jac_maxn | 1) + 64) * sizeof(double) + 64 * sizeof(int);
    if (lds > 48 * 1024)
        PX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_small_psd_project),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (small_sign_maxn > 0 && dev::small_sign_lds_bytes(small_sign_maxn) > 48 * 1024)
        PX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_small_sign_project),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev::small_sign_lds_bytes(small_sign_maxn)));
    PX_HIP(hipStreamSynchronize(stream));
}

// offsets of the 1x1 PSD blocks (clamped by one launch) and of the second-order cones
inline void Solver::setup_soc() {
    if (!one_blocks.empty()) {
        std::vector<long long> offs;
        for (int idx : one_blocks) offs.push_back(P.blocks[idx].off);
        one_off.alloc(offs.size()); one_min.alloc(offs.size());
        one_off.upload(offs.data(), offs.size(), stream);
        PX_HIP(hipStreamSynchronize(stream));
    }
    if (!P.socs.empty()) {
        std::vector<long long> so; std::vector<int> sl;
        for (const SocInfo& S : P.socs) { so.push_back(S.off); sl.push_back(S.len); }
        soc_off.alloc(so.size()); soc_len.alloc(sl.size()); soc_gap_d.alloc(so.size());
        soc_off.upload(so.data(), so.size(), stream); soc_len.upload(sl.data(), sl.size(), stream);
        PX_HIP(hipStreamSynchronize(stream));
    }
}

// the spectral norm and the steps it gives; advanced initialisation.  False: proxsdp_hip_dense_scaling wanted the norm only
inline bool Solver::initial_steps() {
    double spectral_norm = g_frob;                       // LinearAlgebra.norm(M), pdhg.jl:121
    if (!opt.approx_norm) {                              // Arpack.svds(M, nsv=1), pdhg.jl:108-119
        if (P.dense()) spectral_norm = spectral_norm_device();
        else spectral_norm = spectral_norm_host(P, [](int K, double* T, double* d) { return symeig_dense(K, T, d, true); });
        sigma_max = spectral_norm;
    }
    if (init_only) return false;
    if (spectral_norm < 1e-10) spectral_norm = 1.0;
    primal_step = 1.0 / spectral_norm;
    primal_step_old = primal_step;
    dual_step = primal_step;
    std::vector<double> x0;
    if (opt.advanced_initialization) {                   // x = tau*c (pdhg.jl:138-142)
        x0.resize(P.n);
        for (int64_t i = 0; i < P.n; ++i) x0[i] = primal_step * P.c[i];
        xbuf[xc].upload(x0.data(), P.n, stream);
    }
    PX_HIP(hipStreamSynchronize(stream));                // (the set-up is complete; x0 goes out of scope)
    return true;
}

// certificate_infeasibility (pdhg.jl:655-668) / certificate_dual_infeasibility (pdhg.jl:639-653)
inline void Solver::cert_infeas() {
    std::fill(c_host.begin(), c_host.end(), 0.0);
    c_d.zero(stream);
    if (use_support) cS_d.zero(stream);
    cert_zeroed_c = true;
    certificate_parameters();
}
inline void Solver::cert_dual_infeas() {
    std::fill(b_host.begin(), b_host.end(), 0.0);
    std::fill(h_host.begin(), h_host.end(), 0.0);
    rs.bh_d.zero(stream);
    cert_zeroed_bh = true;
    certificate_parameters();
}
inline void Solver::snapshot() { if (req.device_exit) cache_solution_device(false); else cache_solution(P.c_orig); }

// A stop rule fired: record its reason.  True: the loop stops.  False: it goes on -- with certificate search on and no
// search running yet, the search for a certificate of `kind` starts here (data zeroed, limits raised, the point
// snapshotted).  With a search already running the rule stops the loop, except in the limit branch (`at_limit`,
// pdhg.jl:334-382): there a running search neither snapshots nor stops, and the caller re-tests the raised limits.
inline bool Solver::declare(int reason, const std::string& str, Cert kind, bool at_limit) {
    stop_reason = reason;
    stop_reason_string = str;
    if (opt.certificate_search && !certificate_search) {
        if (kind == Cert::infeasible) cert_infeas(); else cert_dual_infeas();
        snapshot();
        return false;
    }
    if (at_limit && opt.certificate_search && certificate_search) return false;
    return true;
}

// dual feasibility of the current y against the cost vector `cvec`: the largest over the shards
inline void Solver::update_dual_feasibility(const std::vector<double>& cvec) {
    std::vector<double> y(P.Q);
    rs.ybuf[yc].download(y.data(), P.Q, stream);
    PX_HIP(hipStreamSynchronize(stream));
    dual_feasibility = dual_feas_host(y, cvec, nullptr, nullptr, nullptr);
    if (sharded()) {                                     // every shard tests its own columns: the model's value is the largest
        std::vector<double> sums, maxs = {dual_feasibility};
        reduce(sums, maxs);
        dual_feasibility = maxs[0];
    }
}

// one iteration of the "CP loop" up to its log line (pdhg.jl:145-183)
inline void Solver::iterate(long long k) {
    const size_t nb = P.blocks.size();
    iter = k;
    lz_matvec_iter = 0; recon_r_iter = 0;
    const double tp0 = now_s();
    primal_step_dev();
    st.t_primal += now_s() - tp0;                    // "primal" section of pdhg.jl:150 (includes t_psd)
    // (the residual / gap REDUCTIONS ride in the candidates' batch and its read-back -- they are part of t_linesearch;
    // t_residual counts what is left of compute_residual! / compute_gap!: the host scalars)
    const double tl0 = now_s();
    const double* s_acc = linesearch_and_residuals();
    const double tl1 = now_s();
    record_residuals(s_acc);
    st.t_linesearch += tl1 - tl0;
    st.t_residual += now_s() - tl1;
    {   // algorithmic bytes of this iteration
        const double t = (double)last_trials;
        double bb = 8.0 * (double)P.n * (11.0 + 3.0 * t) + 12.0 * (double)P.nnz * (1.0 + t) +
                    8.0 * (double)P.Q * (8.0 + 6.0 * t);
        if (P.dense()) {                             // M x + one M'y pass per candidate batch
            dense_ev_harvest();
            bb += 8.0 * (double)P.p * (double)P.n * (double)(st.dense_passes - dense_passes_seen);
            dense_passes_seen = st.dense_passes;
        }
        // per-block L and r are accumulated over blocks in lz_matvec_iter / recon_r_iter;
        // single-block instances (all BASELINE configs) make this exact
        if (nb > 0) {
            const BlockInfo& B0 = P.blocks[0];
            bb += (8.0 * (double)B0.N + 16.0 * (double)B0.n) * (double)lz_matvec_iter +
                  8.0 * (double)B0.n * (double)recon_r_iter;
        }
        st.algorithmic_bytes += bb;
    }
    if (res.trace && res.trace_rows < opt.trace_capacity) {
        double* row = res.trace + (size_t)res.trace_rows * PROXSDP_TRACE_COLS;
        row[0] = (double)k; row[1] = h_pobj.at(k); row[2] = h_dobj.at(k); row[3] = h_gap.at(k);
        row[4] = h_feas.at(k); row[5] = h_pres.at(k); row[6] = h_dres.at(k); row[7] = primal_step;
        row[8] = beta; row[9] = theta; row[10] = nb ? (double)target_rank[0] : 0.0; row[11] = (double)last_trials;
        row[12] = now_s() - loop_t0; row[13] = (double)lz_matvec_iter;
        res.trace_rows++;
    }
    if (opt.check_dual_feas && k % opt.check_dual_feas_freq == 0) {
        std::vector<double> cc(P.c_orig);
        if (stop_reason == 6) std::fill(cc.begin(), cc.end(), 0.0);
        update_dual_feasibility(cc);
    }
    if (opt.log_verbose && opt.log_freq > 0 && k % opt.log_freq == 0)
        std::printf("|%9lld| %+.4e %+.4e %.2e %.2e %.2e %.2e %4lld %8.2f\n", k, h_pobj.at(k), h_dobj.at(k),
                    h_gap.at(k), h_feas.at(k), h_pres.at(k), h_dres.at(k), nb ? target_rank[0] : 0,
                    now_s() - time0);
}

// the stop, rank and step rules after iteration k, in the reference's order (pdhg.jl:184-483; oracle/pdhg.py)
inline Solver::Loop Solver::after_iteration(long long k) {
    const int window = opt.convergence_window;
    const size_t nb = P.blocks.size();
    if (iter < certificate_search_min_iter) return Loop::next;

    if (opt.certificate_search && certificate_search) {          // pdhg.jl:184-244
        if (stop_reason == 6) {
            if (h_dobj.at(k) > opt.certificate_obj_tol) {
                update_dual_feasibility(std::vector<double>(P.n, 0.0));
                if (dual_feasibility < opt.tol_feasibility_dual) {
                    certificate_found = true;
                    stop_reason_string += " [Dual ray found]";
                    return Loop::stop;
                }
            }
        } else {
            if (h_pobj.at(k) < -opt.certificate_obj_tol && h_feas.at(iter) < opt.tol_feasibility) {
                certificate_found = true;
                stop_reason_string += " [Primal ray found]";
                return Loop::stop;
            }
        }
        if ((h_pobj.at(k) < -opt.certificate_fail_tol && h_dobj.at(k) < -opt.certificate_fail_tol &&
             h_feas.at(iter) < -opt.certificate_fail_tol) || std::isnan(h_comb.at(k))) {
            stop_reason_string += " [Failed to find certificate]";
            return Loop::stop;
        }
    }

    // ---- convergence / rank update / divergence / adaptive steps (pdhg.jl:246-332)
    rank_update += 1;
    if (h_gap.at(iter) <= opt.tol_gap && h_feas.at(iter) <= opt.tol_feasibility &&
        (!opt.check_dual_feas || dual_feasibility < opt.tol_feasibility_dual)) {
        if ((sharded() ? !g_not_converged_rank : convergedrank()) && soc_convergence() && iter > opt.min_iter) {
            if (!certificate_search) {
                stop_reason = 1;
                stop_reason_string = "Optimal solution found";
            } else {
                stop_reason_string += " [Failed to find certificate - type 2]";
            }
            return Loop::stop;
        } else if (rank_update > window) {
            update_cont += 1;
            if (update_cont > 0) {
                for (size_t idx = 0; idx < nb; ++idx) bump_rank((int)idx);
                rank_update = 0; update_cont = 0;
            }
        }
    } else if (k > window && h_comb.at(k - window) < h_comb.at(k) && rank_update > window) {
        update_cont += 1;
        if (update_cont > opt.divergence_min_update) {
            if (sharded() && g_any_below_full) { rank_update = 0; update_cont = 0; }
            for (size_t idx = 0; idx < nb; ++idx) {
                if (target_rank[idx] < P.blocks[idx].n) { rank_update = 0; update_cont = 0; }
                bump_rank((int)idx);
            }
        }
    } else if (h_pres.at(k) > opt.tol_primal && h_dres.at(k) < opt.tol_dual && k > window) {
        if (++ada_count > opt.adapt_window) {
            ada_count = 0;
            if (opt.line_search_flag) { beta *= (1.0 - adapt_level); primal_step /= std::sqrt(1.0 - adapt_level); }
            else { primal_step /= (1.0 - adapt_level); dual_step *= (1.0 - adapt_level); }
            adapt_level *= opt.adapt_decay;
        }
    } else if (h_pres.at(k) < opt.tol_primal && h_dres.at(k) > opt.tol_dual && k > window) {
        if (++ada_count > opt.adapt_window) {
            ada_count = 0;
            if (opt.line_search_flag) { beta /= (1.0 - adapt_level); primal_step *= std::sqrt(1.0 - adapt_level); }
            else { primal_step *= (1.0 - adapt_level); dual_step /= (1.0 - adapt_level); }
            adapt_level *= opt.adapt_decay;
        }
    }

    // ---- iteration / time limits (pdhg.jl:334-382)
    const double elapsed = sharded() ? g_elapsed : now_s() - time0;
    if (iter >= max_iter_local || elapsed >= time_limit) {
        if (iter > opt.min_iter_time_infeas && h_gap.max_abs_diff() < opt.infeas_stable_gap_tol &&
            h_gap.at(k) > opt.infeas_limit_gap_tol) {
            if (h_feas.at(iter) <= opt.tol_feasibility / 100) {
                if (declare(5, "Problem declared unbounded due to lack of improvement", Cert::dual_infeasible, true))
                    return Loop::stop;
            } else if (h_feas.at(iter) > opt.infeas_feasibility_tol) {
                if (declare(6, "Problem declared infeasible due to lack of improvement", Cert::infeasible, true))
                    return Loop::stop;
            }
        } else if (iter >= max_iter_local) {
            stop_reason = 3;
            stop_reason_string = "Iteration limit of " + std::to_string(max_iter_local) + " was hit";
        } else {
            stop_reason = 2;
            stop_reason_string = "Time limit hit, limit: " + std::to_string(time_limit) +
                                 " time: " + std::to_string(now_s() - time0);
        }
        // (a search that began just above raised both limits: the same elapsed time against the new ones)
        if (iter >= max_iter_local || elapsed >= time_limit) return Loop::stop;
    }
    if (opt.certificate_search && certificate_search) return Loop::next;

    // ---- objective blow-up / stalls (pdhg.jl:389-483)
    if ((iter > opt.min_iter_max_obj && h_dobj.at(k) > opt.max_obj) || std::isnan(h_dobj.at(k))) {
        if (declare(6, "Infeasible: |Dual objective| = " + std::to_string(h_dobj.at(k)) +
                       " > maximum allowed = " + std::to_string(opt.max_obj), Cert::infeasible))
            return Loop::stop;
    }
    if ((iter > opt.min_iter_max_obj && h_pobj.at(k) < -opt.max_obj) || std::isnan(h_pobj.at(k))) {
        if (declare(5, "Unbounded: |Primal objective| = " + std::to_string(h_pobj.at(k)) +
                       " > maximum allowed = " + std::to_string(opt.max_obj), Cert::dual_infeasible))
            return Loop::stop;
    }
    if (iter > opt.min_iter_max_obj && h_gap.at(k) > opt.infeas_limit_gap_tol &&
        h_feas.at(iter) > opt.infeas_feasibility_tol &&
        h_feas.max_abs_diff() < opt.infeas_stable_feasibility_tol) {
        if (declare(6, "Infeasible: feasibility stalled at " + std::to_string(h_feas.at(iter)), Cert::infeasible))
            return Loop::stop;
    }
    if (iter > opt.min_iter_max_obj && h_gap.at(k) > 1 - opt.infeas_gap_tol &&
        h_gap.max_abs_diff() < opt.infeas_stable_gap_tol) {
        if (std::fabs(h_dobj.at(k)) > std::fabs(h_pobj.at(k)) && h_feas.at(iter) > opt.infeas_feasibility_tol) {
            if (declare(6, "Infeasible: duality gap stalled at 100 % with |Dual objective| >> |Primal objective|", Cert::infeasible))
                return Loop::stop;
        } else if (std::fabs(h_pobj.at(k)) > std::fabs(h_dobj.at(k)) && h_feas.at(iter) <= opt.tol_feasibility) {
            if (declare(5, "Unbounded: duality gap stalled at 100 % with |Dual objective| << |Primal objective|", Cert::dual_infeasible))
                return Loop::stop;
        }
    }
    return Loop::next;
}

// after the loop: pending capture, event harvest, the solution (pdhg.jl:486-529), debug summaries
inline void Solver::finish() {
    PX_HIP(hipStreamSynchronize(stream));
    if (req.capture_state && req.capture_state->ints[3] == 0 && iter == req.capture_state->iteration) write_capture();
    for (EigWork& W : eig) harvest_full_eig_events(W);
    merge_block_stats();
    st.loop_time = now_s() - loop_t0;
    if (warm.joinable()) warm.join();

    // ---- results (pdhg.jl:486-529)
    if (opt.certificate_search && certificate_search) {
        if (certificate_found) {
            if (req.device_exit) {
                cache_solution_device(stop_reason == 6);
            } else {
                std::vector<double> cc(P.c_orig);
                if (stop_reason == 6) std::fill(cc.begin(), cc.end(), 0.0);
                cache_solution(cc);
            }
        }
    } else if (req.device_exit) {
        cache_solution_device(false);
    } else {
        cache_solution(P.c_orig);
    }
    if (debug && dbg_lz.cycles > 0)
        std::fprintf(stderr, "[proxsdp] single-block Lanczos: %.0f cycles; per cycle: wait for the GPU %.1f us | after-cycle host logic (eigensolve, "
                     "convergence, restart rotation staging) %.1f us; per projection: results (Ritz coefficients + rotation staging) %.1f us\n",
                     dbg_lz.cycles, 1e6 * dbg_lz.wait / dbg_lz.cycles, 1e6 * dbg_lz.after_cycle / dbg_lz.cycles, 1e6 * dbg_lz.results / std::max(1.0, (double)st.lanczos_calls));
    if (b1_dbg.p != nullptr) {
        long long t[8] = {0};
        b1_dbg.download(t, 8, stream);
        PX_HIP(hipStreamSynchronize(stream));
        if (t[4] > 0)
            std::fprintf(stderr, "[proxsdp] k_lz_block1: %lld launches, %lld steps; per launch: prologue %.2f us | step loop %.2f us (%.2f us per step) | "
                         "epilogue %.2f us\n", t[4], t[3], 0.01 * t[0] / t[4], 0.01 * t[1] / t[4], 0.01 * t[1] / std::max(1LL, t[3]), 0.01 * t[2] / t[4]);
    }
    if (debug && dbg_batch.cycles > 0)
        std::fprintf(stderr, "[dbg] batched Lanczos: %.0f cycles; per cycle enqueue %.1f us, wait %.1f us, restart logic %.1f us, flush %.1f us\n",
                     dbg_batch.cycles, 1e6 * dbg_batch.enqueue / dbg_batch.cycles, 1e6 * dbg_batch.wait / dbg_batch.cycles,
                     1e6 * dbg_batch.restart / dbg_batch.cycles, 1e6 * dbg_batch.flush / dbg_batch.cycles);
    res.stats = st;
}

inline void Solver::run() {
    setup();
    solve();
}

// everything before the first step size: what a model handle (model.hip.hpp) runs once
inline void Solver::setup() {
    t_init0 = now_s();
    check_run_options();
    init_parameters();
    reduce_global_constants();

    // ---- device state ("Init", pdhg.jl:54-142)
    setup_device();
    setup_dense_scaling();                               // (equilibration on a dense A: finishes what prepare() deferred)
    b_host = P.b; h_host = P.h; c_host = P.c;
    start_host_helpers();
    alloc_iterate();
    upload_sparse_operator();
    classify_blocks();
    start_block_workers();
    setup_small_batch();
    setup_soc();
    if (P.dense()) opt.support_path = 0;                 // every column of a dense M is in the support
    setup_support();                                     // (a block-sharded solve chose opt.support_path in classify_blocks)
    setup_dense();
    alloc_candidates();
    if (sharded() && use_support == shard_general)
        throw std::logic_error("block-sharded solve: the shard's vector path is not the one chosen for it");
}

// the steps, the start path, the loop and the exit: what a model handle runs per solve
inline void Solver::solve() {
    if (!initial_steps()) return;

    // ---- where the loop enters: cold, resumed (proxsdp_hip_solve_ex) or from the caller's point (proxsdp_hip_solve_from)
    long long k_first = 1;
    if (req.resume_state) { apply_resume(); k_first = req.resume_state->iteration + 1; }
    if (req.start_point()) apply_start();
    if (req.start_out) { write_start_point(); return; }
    if (req.capture_state) { check_state_shape(*req.capture_state, "capture"); req.capture_state->ints[3] = 0; }
    st.init_time = now_s() - t_init0;

    // ---- "CP loop" (pdhg.jl:145-484)
    loop_t0 = now_s();
    const long long kmax = 2 * max_iter_local;
    for (long long k = k_first; k <= kmax; ++k) {
        if (req.capture_state && k == req.capture_state->iteration + 1 && k > k_first) write_capture();
        iterate(k);
        if (after_iteration(k) == Loop::stop) break;
    }
    finish();
}

// ---- a solver kept set up between solves (model.hip.hpp)
// One block's workspace as classify_blocks() and setup_support() left it: the buffers they zeroed are zero again (and the
// ones a run fills before it reads them as well: the same launch costs nothing more), the start vector is uploaded again,
// every host member a projection writes has its initial value.  What the set-up built stays: sizes, the record pointers,
// the ELL structures with fop_ok, the streams and events, the sign projection's work matrices with their tile shape
// (allocated on first use; sgA's padding is zero and stays zero, as the rows the 48-tiles never write).
inline void Solver::reset_eigwork(EigWork& W) {
    for (DevBuf<double>* b : {&W.V, &W.Z, &W.w, &W.Ppart, &W.hpart1, &W.hpart2, &W.hsum1, &W.hred, &W.U, &W.lam, &W.Apart,
                              &W.arrow, &W.rec, &W.hpw1, &W.hpw2, &W.hsw1, &W.hsw2, &W.recw, &W.F, &W.Flam, &W.tpart, &W.tred,
                              &W.ebuf, &W.apartf, &W.warm_part, &W.sg_sc, &W.sg_part, &W.sg_part2})
        b->zero(stream);
    if (W.resid.n > 0) W.resid.upload(W.resid_host.data(), W.npad, stream);
    if (W.arrow_host.p) std::fill(W.arrow_host.p, W.arrow_host.p + 2 * dev::MAXK, 0.0);
    static_cast<EigSolveState&>(W) = EigSolveState{};    // every per-solve host member (the rule is at the struct)
    W.arrow_p = W.arrow.p;                               // (its value comes from the set-up)
    // owners of buffers, events and a helper pool that stay: only their per-solve fields
    W.split.k1 = 0; W.split.K = 0; W.split.beta = 0.0; W.split.have_first = false; W.split.M.par = nullptr;
    W.ev.used = 0; W.evo.used = 0;
}

// [b; h] as one host vector of P.Q entries (scaled or the caller's: the loop's and the exit path's uploads)
inline std::vector<double> Solver::stacked_bh(const std::vector<double>& b, const std::vector<double>& h) const {
    std::vector<double> bh((size_t)P.Q);
    std::copy(b.begin(), b.begin() + P.p, bh.begin());
    std::copy(h.begin(), h.begin() + P.m, bh.begin() + P.p);
    return bh;
}

// c and [b; h] on the device after a certificate search zeroed them (cert_infeas, cert_dual_infeas): from the Prep again
inline void Solver::restore_cert_data() {
    if (cert_zeroed_c) {
        c_host = P.c;
        c_d.upload(P.c.data(), P.n, stream);
        if (use_support) {
            std::vector<double> cS(std::max(ns, 1), 0.0);
            for (int s = 0; s < ns; ++s) cS[s] = P.c[supp_h[s]];
            cS_d.upload(cS.data(), ns, stream);
            PX_HIP(hipStreamSynchronize(stream));        // (cS goes out of scope)
        }
        cert_zeroed_c = false;
    }
    if (cert_zeroed_bh) {
        b_host = P.b; h_host = P.h;
        const std::vector<double> bh = stacked_bh(P.b, P.h);
        rs.bh_d.upload(bh.data(), P.Q, stream);
        PX_HIP(hipStreamSynchronize(stream));
        cert_zeroed_bh = false;
    }
}

// Every member a solve writes, back at the value it has after setup().  The data vectors a certificate search zeroes
// (cert_infeas, cert_dual_infeas) come back from the Prep, which a model handle keeps current.
inline void Solver::reset_for_solve() {
    PX_HIP(hipStreamSynchronize(stream));
    static_cast<SolveState&>(*this) = SolveState{};      // every per-solve host scalar (the rule is at the struct)
    req = SolveRequest{};                                // the one place a request is cleared
    init_parameters();                                   // Params, target ranks, histories, time_limit
    reduce_global_constants();                           // the norms may have changed (proxsdp_hip_model_update); max_iter_local
    for (int k = 0; k < 2; ++k) { xbuf[k].zero(stream); Mtybuf[k].zero(stream); rs.ybuf[k].zero(stream); rs.Mxbuf[k].zero(stream); }
    restore_cert_data();
    part.zero(stream); scal.zero(stream);
    small_rank.zero(stream);
    if (small_rank_host.p) std::fill(small_rank_host.p, small_rank_host.p + 2 * small_blocks.size() + 2, 0.0);
    if (use_support) { MtyS_cur.zero(stream); xsave_d.zero(stream); esv_d.zero(stream); respart_d.zero(stream); }
    rs.ycand_d.zero(stream); Mtycand_d.zero(stream); bpart.zero(stream); bscal.zero(stream);
    hbscal.assign(64, 0.0);
    if (hscal_pin.p) std::fill(hscal_pin.p, hscal_pin.p + 64, 0.0);
    for (int idx : big_blocks) reset_eigwork(eig[idx]);
    batch_ctx.clear();                                   // (the batched runs' buffers come on first use, as in a fresh solve)
    PX_HIP(hipStreamSynchronize(stream));
}

// the block workers and the merge helpers end with a solve: a model handle keeps no thread between calls
inline void Solver::release_host_threads() {
    block_pool.reset();
    merge_pool.reset();
    for (auto& c : batch_ctx) if (c) c->pool.reset();
}

}  // namespace proxsdp
