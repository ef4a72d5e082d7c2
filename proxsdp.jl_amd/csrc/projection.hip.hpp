// psd_projection! (prox_operators.jl:33-126): which engine projects which block.  The engines themselves are lanczos.hip.hpp (lanczos*) and
// solver.hip.hpp (full_eig_by_sign, full_eig_values, launch_reconstruct, the sym_gemm family); this file only decides,
// in call order: the cone's blocks, one block, the Krylov branch, the full_eig! branch, the dense engines.
#pragma once
#include "solver.hip.hpp"

namespace proxsdp {

inline void Solver::psd_projection(double* x) {
    std::fill(min_eig.begin(), min_eig.end(), 0.0);
    if (!one_blocks.empty()) {
        launch_clamp_scalars(x, (int)one_blocks.size());
        for (int idx : one_blocks) current_rank[idx] = 0;
    }
    if (!small_blocks.empty()) {
        project_small_blocks(x);
        project_blocks(large_blocks, x, x, false);
    } else {
        project_blocks(big_blocks, x, x, false);
    }
}

// all small PSD blocks in one launch (kernels.hip.hpp k_small_psd_project); ranks come back with the
// iteration's next synchronisation (pinned buffer)
inline void Solver::project_small_blocks(double* x) {
    harvest_small_ranks();
    const int nb = (int)small_blocks.size();
    // ranks, positive counts, the schedule-test outcomes and the Jacobi sweep counts [nb each] go STRAIGHT into pinned host memory (no copy launch)
    // (small models only, as the scalars of the linesearch: zero_copy_small; otherwise through the device buffer and one copy)
    const bool zc = zero_copy_small();
    int* rk_host = zc ? reinterpret_cast<int*>(small_rank_host.p) : small_rank.p;
    if (zc) for (int q = 0; q < nb; ++q) { rk_host[2 * nb + q] = 0; rk_host[3 * nb + q] = -1; }   // (the previous launch's values were harvested above)
    else {
        PX_HIP(hipMemsetAsync(small_rank.p + 2 * nb, 0, (size_t)nb * sizeof(int), stream));
        PX_HIP(hipMemsetAsync(small_rank.p + 3 * nb, 0xFF, (size_t)nb * sizeof(int), stream));      // (-1: not a Jacobi block)
    }
    bool any_jacobi = false;
    int jac_maxn = 0;
    for (int idx : small_blocks) if (P.blocks[idx].n <= small_jacobi_max) { any_jacobi = true; jac_maxn = std::max(jac_maxn, P.blocks[idx].n); }
    if (any_jacobi) {
        const int ld = jac_maxn | 1;
        const size_t lds = ((size_t)2 * jac_maxn * ld + 64) * sizeof(double) + 64 * sizeof(int);
        hipLaunchKernelGGL(dev::k_small_psd_project, dim3(nb), dim3(dev::TPB), lds, stream,
                           x, (const long long*)small_off.p, (const int*)small_side.p, opt.tol_psd, rk_host, rk_host + nb,
                           2, small_jacobi_max, rk_host + 3 * nb);
    }
    if (small_sign_maxn > 0) {
        // shortened, tested schedule as Solver::full_eig_by_sign: start at row 8 (sign_start_row overrides), fall back inside the kernel
        static const dev::SignSchedule sched;
        const int jmax = sched.max_start_row(4e-13 * (double)dev::SS_MAXN);   // (the test's tau at the largest side)
        const int j0 = std::max(0, std::min(opt.sign_start_row < 0 ? 8 : (int)opt.sign_start_row, jmax));
        hipLaunchKernelGGL(dev::k_small_sign_project, dim3(nb), dim3(dev::SS_TPB), dev::small_sign_lds_bytes(small_sign_maxn), stream,
                           x, (const long long*)small_off.p, (const int*)small_side.p, small_jacobi_max + 1, dev::SS_MAXN,
                           rk_host, rk_host + nb, j0, sched.fallback_row(j0), j0 > 0 ? rk_host + 2 * nb : (int*)nullptr);
        st.full_eigs_sign += nb; st.sign_products += 57LL * nb;      // (counted per block below for the Jacobi ones)
        for (int idx : small_blocks) if (P.blocks[idx].n <= small_jacobi_max) { st.full_eigs_sign--; st.sign_products -= 57; }
    }
    if (!zc) PX_HIP(hipMemcpyAsync(small_rank_host.p, small_rank.p, (size_t)4 * nb * sizeof(int), hipMemcpyDeviceToHost, stream));
    small_pending = true;
    st.full_eigs += nb; st.batched_small_eigs += nb;
    for (int idx : small_blocks) { current_rank[idx] = 0; min_eig[idx] = 0.0; }
}
// (called after a stream synchronisation has happened since the launch: every iteration ends with one)
inline void Solver::harvest_small_ranks() {
    if (!small_pending) return;
    small_pending = false;
    const int* r = reinterpret_cast<const int*>(small_rank_host.p);
    for (size_t q = 0; q < small_blocks.size(); ++q) {
        if (r[q] < 0) throw HipError("projection of a small block (one-launch Jacobi or sign function) produced non-finite values");
        current_rank[small_blocks[q]] = r[q];
    }
    small_sweeps.assign(r + 3 * small_blocks.size(), r + 4 * small_blocks.size());   // (Jacobi blocks: sweeps run; the others -1)
    // the shortened schedule's tests made inside k_small_sign_project (cumulative counters behind the ranks)
    const int* flag = r + 2 * small_blocks.size();            // per block: 1 = test passed, 2 = failed (fall-back rows ran), 0 = no test
    for (size_t q = 0; q < small_blocks.size(); ++q) { st.sign_short_pass += flag[q] == 1; st.sign_short_fail += flag[q] == 2; }
}

// psd_projection!'s loop over the blocks (prox_operators.jl:40-61): blocks of equal side whose Lanczos runs can
// be batched go through ONE launch per step (groups of up to LZB_MAX), the rest through run_blocks
// (one stream + host thread per block, or in sequence)
inline void Solver::project_blocks(const std::vector<int>& blocks, const double* xin, double* xout, bool fuse) {
    std::vector<int> rest;
    std::vector<std::vector<int>> groups;
    // (groups run side by side only ON REQUEST -- block_batch_groups >= 2; a model with more than LZB_MAX equal-side
    // blocks splits into several groups by necessity, and those run one after the other as in rounds 3-4: auto = sequential)
    const int want_groups = opt.block_batch_groups < 0 ? 1 : (int)opt.block_batch_groups;   // (auto = 1: measured, see the header)
    if (opt.block_batch != 0 && blocks.size() >= 2) {
        std::vector<int> cand;
        for (int idx : blocks) (batch_eligible(idx, fuse) ? cand : rest).push_back(idx);
        std::stable_sort(cand.begin(), cand.end(), [this](int a, int b) { return eig[a].n < eig[b].n; });
        size_t i0 = 0;
        while (i0 < cand.size()) {
            size_t i1 = i0;
            while (i1 < cand.size() && eig[cand[i1]].n == eig[cand[i0]].n) ++i1;
            // equal-side run [i0, i1): groups of up to LZB_MAX blocks; with the worker pool up, at least two groups of >= 2
            // blocks on request (options.block_batch_groups) so that they can overlap
            const size_t cnt = i1 - i0;
            if (cnt < 2) { rest.push_back(cand[i0]); i0 = i1; continue; }
            size_t ng = (cnt + dev::LZB_MAX - 1) / dev::LZB_MAX;
            if (parallel_blocks() && want_groups >= 2 && cnt >= 4) ng = std::max<size_t>(ng, std::min<size_t>((size_t)want_groups, cnt / 2));
            for (size_t q = 0; q < ng; ++q) {
                const size_t a = i0 + q * cnt / ng, b = i0 + (q + 1) * cnt / ng;
                groups.emplace_back(cand.begin() + a, cand.begin() + b);
            }
            i0 = i1;
        }
        std::sort(rest.begin(), rest.end());
    } else {
        rest = blocks;
    }
    // groups run CONCURRENTLY when the block worker pool is up (one worker thread + the leader block's stream per group):
    // while one group's restart logic runs on the host the other group's cycle runs on the GPU (the step launches are
    // latency-bound: two groups side by side advance about as fast as one).  Per block nothing changes.
    if (batch_ctx.size() < groups.size()) {
        const size_t have = batch_ctx.size();
        batch_ctx.resize(groups.size());
        for (size_t q = have; q < groups.size(); ++q) batch_ctx[q].reset(new BatchCtx());
    }
    for (const std::vector<int>& g : groups) for (int idx : g) current_rank[idx] = 0;
    auto run_group = [this, xin, &groups](int q) {
        std::vector<int> nevs;
        for (int idx : groups[q]) nevs.push_back((int)target_rank[idx]);
        lanczos_batch(groups[q], xin, nevs, q);
    };
    bool leaders_have_streams = parallel_blocks() && groups.size() >= 2 && want_groups >= 2;
    for (const std::vector<int>& g : groups) leaders_have_streams = leaders_have_streams && eig[g[0]].stream != nullptr;
    if (leaders_have_streams) {
        std::vector<int> leaders;
        std::vector<int> slot_of(eig.size(), -1);
        for (size_t q = 0; q < groups.size(); ++q) { leaders.push_back(groups[q][0]); slot_of[groups[q][0]] = (int)q; }
        run_blocks(leaders, [&run_group, &slot_of](int leader) { run_group(slot_of[leader]); });
    } else {
        for (size_t q = 0; q < groups.size(); ++q) run_group((int)q);
    }
    // a batched run has filled W.vals / W.Z from the packed operator (no operator form, nothing to count for it)
    for (const std::vector<int>& g : groups)
        for (int idx : g) {
            EigWork& W = eig[idx];
            W.ritz_ok = false;                        // the block is about to be rewritten
            W.use_fop = false;
            finish_krylov_run(idx, xin + P.blocks[idx].off, xout + P.blocks[idx].off, fuse, (int)target_rank[idx]);
        }
    if (!groups.empty()) merge_block_stats();
    if (!rest.empty()) run_blocks(rest, [this, xin, xout, fuse](int idx) { project_block(idx, xin, xout, fuse); });
}

// the branch condition of psd_projection! (prox_operators.jl:46-49)
inline bool Solver::krylov_branch(int idx) const {
    return !opt.full_eig_decomp && target_rank[idx] <= opt.max_target_rank_krylov_eigs &&
           eig[idx].n > opt.min_size_krylov_eigs && (iter % opt.full_eig_freq) > opt.full_eig_len;
}
// may this block's Lanczos run ride in a batched launch (lanczos.hip.hpp lanczos_batch)?
inline bool Solver::batch_eligible(int idx, bool fuse) const {
    if (opt.block_batch == 0 || !krylov_branch(idx)) return false;
    if (opt.eigsolver == 1 || opt.psd_sign_engine == 1 || opt.lanczos_warm_start > 0 || opt.krylovkit_eager)
        return false;
    // operator-form blocks keep their own path (their step kernels take per-block factor ranks)
    if (fop_eligible(eig[idx], fuse)) return false;
    return krylov_dim((int)target_rank[idx]) <= 63;
}
// operator-form mat-vec: legal when this block's x_prev is known in factored form (or is
// zero off the support) and the update is the sparse support update of this iteration
inline bool Solver::fop_eligible(const EigWork& W, bool fuse) const {
    return fuse && use_support && opt.lanczos_operator != 0 && W.fop_ok && (W.have_factors || W.xprev.sparse);
}
// ... and what its kernels read: the factors' columns (none for an x_prev that is zero off the support), the support values
inline void Solver::arm_fop(EigWork& W) {
    if (!W.have_factors) { W.F_r = 0; W.F_first = 0; }
    W.esv = esv_d.p + (W.have_factors ? 0 : ns);
}

// psd_projection! (prox_operators.jl:33-66), one block: reads the packed block of xin,
// writes the projected block into xout (xin == xout on the dense path)
inline void Solver::project_block(int idx, const double* xin, double* xout, bool fuse) {
    EigWork& W = eig[idx];
    const double* xp = xin + P.blocks[idx].off;
    double* xo = xout + P.blocks[idx].off;
    current_rank[idx] = 0;
    W.ritz_ok = false;                        // the block is about to be rewritten
    W.use_fop = false;                        // (until a branch below arms the operator form)
    const int nev = (int)target_rank[idx];
    if (!krylov_branch(idx)) { full_eig_branch(idx, xp, xo, fuse); return; }
    // (a Krylov dimension beyond the step kernels -- the wide kernels or the dense stand-in -- takes the packed-tile mat-vec)
    W.use_fop = fop_eligible(W, fuse) && !(opt.krylovkit_eager && opt.eigsolver != 1) && krylov_dim(nev) <= dev::LZ_KMAX;
    if (W.use_fop) arm_fop(W);
    if (!krylovdim_fits(nev)) {               // Krylov dimension beyond the step kernels: dense eigensolver, same projection
        W.use_fop = false;
        truncated_project_dense(idx, xp, xo, fuse, nev);
        return;
    }
    krylov_run(idx, xp, xo, fuse, nev);
}

// full_eig! (prox_operators.jl:111-126): every positive eigenpair.  In the IMPLICIT full-eig
// regime (target_rank beyond max_target_rank_krylov_eigs: the reference falls back to LAPACK
// because its Krylov wrapper is capped, prox_operators.jl:46-49) the positive part is
// low-rank and known from the previous projection: it is computed by the Lanczos engine
// (operator form allowed) instead of a dense O(n^3) eigensolver -- see full_eig_by_lanczos.
// An explicit full_eig_decomp = true / periodic full_eig_freq request always gets the dense solver.
inline void Solver::full_eig_branch(int idx, const double* xp, double* xo, bool fuse) {
    EigWork& W = eig[idx];
    const bool implicit = !opt.full_eig_decomp && (iter % opt.full_eig_freq) > opt.full_eig_len &&
                          W.n > opt.min_size_krylov_eigs;
    if (implicit || opt.full_eig_lanczos == 1) {
        W.use_fop = fop_eligible(W, fuse);
        if (W.use_fop) arm_fop(W);
        if (full_eig_by_lanczos(idx, xp, xo, fuse)) return;
    }
    W.forget_factors();
    full_eig_project(idx, xp, xo, fuse);
}

// the Krylov branch (prox_operators.jl:68-109) on the step or wide kernels: the sign stand-in where it is the cheaper way to
// the same matrix, else the Lanczos run
inline void Solver::krylov_run(int idx, const double* xp, double* xo, bool fuse, int nev) {
    EigWork& W = eig[idx];
    const bool used_fop = W.use_fop;
    if (exact_projection_by_sign(idx, xp, xo, fuse, nev)) return;
    const double t_kry = opt.psd_sign_engine == 1 ? now_s() : 0.0;
    lanczos(W, xp, nev);
    if (opt.psd_sign_engine == 1 && W.converged) {
        const double ms = (now_s() - t_kry) * 1e3;
        W.sign.kry_ms = W.sign.kry_ms < 0 ? ms : 0.75 * W.sign.kry_ms + 0.25 * ms;
    }
    W.use_fop = false;
    if (used_fop) W.lst.fop_projections++;
    finish_krylov_run(idx, xp, xo, fuse, nev);
}

// what follows a Lanczos run of the Krylov branch (Solver::lanczos, or lanczos_batch for several blocks at once): the
// reference's fallback when it did not converge, else the positive ones among the converged pairs rebuild the block
inline void Solver::finish_krylov_run(int idx, const double* xp, double* xo, bool fuse, int nev) {
    EigWork& W = eig[idx];
    if (!W.converged) {                       // prox_operators.jl:55-57
        W.lst.krylov_fallbacks++;
        W.forget_factors();
        full_eig_project(idx, xp, xo, fuse);
        return;
    }
    double mn = W.vals[0];
    for (double v : W.vals) mn = std::min(mn, v);
    min_eig[idx] = mn;                        // prox_operators.jl:95 / :74
    int first = 0, npos = 0;
    if (opt.eigsolver == 1) {                 // ascending arc.d, all nev used (prox_operators.jl:78-85)
        for (int i = 0; i < nev; ++i) if (W.vals[i] > 0.0) ++npos;
        first = nev - npos;
    } else {                                  // descending, min(target_rank, converged) used (:99-106)
        const int k = std::min(nev, W.converged_eigs);
        for (int i = 0; i < k; ++i) if (W.vals[i] > 0.0) ++npos;
    }
    current_rank[idx] += npos;
    W.xprev.last_npos = npos;                 // (lower bound: estimate for a later full_eig!-by-Lanczos)
    ritz_pairs_to_block(idx, xp, xo, fuse, first, npos);
    if (W.sign.check_pending) verify_sign_engine(idx, xo);
}

// the block from the Ritz pairs Z[:, first .. +npos), vals[first ..) of the run that just ended; the pairs are kept as the
// factored form of the new x_prev
inline void Solver::ritz_pairs_to_block(int idx, const double* xp, double* xo, bool fuse, int first, int npos) {
    EigWork& W = eig[idx];
    if (npos > 0) W.lam.upload(W.vals.data() + first, npos, stream);
    launch_reconstruct(W, W.Z.p + (size_t)first * W.npad, W.npad, W.lam.p, npos, xo,
                       fuse ? xp : nullptr, fuse ? idx : -1);
    W.recon_r += npos;
    if (W.fop_ok) {                           // x_new = Z[:, first..] diag(lam) Z': keep the factors
        std::swap(W.Z.p, W.F.p);
        W.F_first = first; W.F_r = npos;
        std::swap(W.lam.p, W.Flam.p);            // the eigenvalues just uploaded become the next projection's factors
        std::swap(W.lam.n, W.Flam.n);
        W.have_factors = true; W.xprev.sparse = false;
    } else {                                  // no F to swap into: the pairs stay in Z / vals (extract_factors)
        W.ritz_first = first; W.ritz_r = npos; W.ritz_ok = true;
    }
}

// A SHADOW projection: another engine projects the same input into W.sg_out without touching the block's bookkeeping.  While
// one of these lives the caller runs that engine and reads what it found; the destructor puts back the rank, min_eig, what is
// known of x_prev and the full_eig! counts (the check is not a full_eig! call of the solve).
struct Solver::ShadowBookkeeping {
    Solver& S; EigWork& W; const int idx;
    const long long rank; const double min_eig; const int last_npos; const bool have_factors, sparse, use_fop;
    const long long full_eigs, full_eigs_sign;
    ShadowBookkeeping(Solver& s, int i)
        : S(s), W(s.eig[i]), idx(i), rank(s.current_rank[i]), min_eig(s.min_eig[i]), last_npos(W.xprev.last_npos),
          have_factors(W.have_factors), sparse(W.xprev.sparse), use_fop(W.use_fop), full_eigs(W.lst.full_eigs),
          full_eigs_sign(W.lst.full_eigs_sign) {
        if (W.sg_out.n < (size_t)W.N) W.sg_out.alloc(W.N);
    }
    ~ShadowBookkeeping() {
        S.current_rank[idx] = rank; S.min_eig[idx] = min_eig; W.xprev.last_npos = last_npos;
        W.have_factors = have_factors; W.xprev.sparse = sparse; W.use_fop = use_fop;
        W.lst.full_eigs = full_eigs; W.lst.full_eigs_sign = full_eigs_sign;
    }
};
// does the block at xo agree with the shadow in W.sg_out?  (max |difference| <= 1e-8 max |value|; one synchronisation)
inline bool Solver::matches_shadow(EigWork& W, const double* xo) {
    if (W.sg_cmp.n < 2) W.sg_cmp.alloc(2);
    W.sg_cmp.zero(stream);
    hipLaunchKernelGGL(dev::k_maxdiff, dim3(grid_for(W.N)), dim3(dev::TPB), 0, stream, xo, (const double*)W.sg_out.p,
                       (long long)W.N, W.sg_cmp.p);
    double h[2] = {0.0, 0.0};
    W.sg_cmp.download(h, 2, stream);
    PX_HIP(hipStreamSynchronize(stream));
    return h[0] <= 1e-8 * std::max(h[1], 1e-300);
}

// psd_sign_engine = 1: the Krylov branch computes the top target_rank eigenpairs and keeps the positive ones
// (prox_operators.jl:89-109).  Whenever fewer than target_rank eigenvalues are positive that IS the exact
// projection, min_eig (the smallest returned value) is <= 0, and the two decisions min_eig feeds
// (pdhg.jl:272 `> tol_psd`, residuals.jl:93 `< tol_psd`) are settled -- so the sign-function projection
// (sign_project.hip.hpp) may stand in for the Lanczos engine when it is the cheaper way to the same matrix:
// hub-row / clustered spectra that cost hundreds of mat-vecs per projection (maxG51: 541), many mid-size
// blocks (MIMO).  It is chosen per block from measured wall-clock averages of both engines, only when the
// previous projection was not truncated, and VERIFIED afterwards: #{lambda > 0} >= target_rank means the
// reference would have truncated, and the projection is redone by the Lanczos engine.
inline double sign_cost_model_ms(int ld) {                   // measured on MI355X (profiles/r02c_sign_projection_summary.md)
    static const int L[] = {128, 512, 1024, 1536, 2048, 3072, 4096};
    static const double T[] = {0.30, 0.60, 2.05, 4.8, 11.3, 31.2, 71.2};
    if (ld <= L[0]) return T[0];
    for (int i = 1; i < 7; ++i)
        if (ld <= L[i]) return T[i - 1] + (T[i] - T[i - 1]) * (double)(ld - L[i - 1]) / (L[i] - L[i - 1]);
    return T[6] * std::pow((double)ld / 4096.0, 3.0);
}
inline bool Solver::exact_projection_by_sign(int idx, const double* xp, double* xo, bool fuse, int nev) {
    if (opt.psd_sign_engine != 1) return false;
    EigWork& W = eig[idx];
    EigWork::SignStandIn& S = W.sign;
    S.check_pending = false;                                              // (a verification whose Lanczos half fell back)
    if (W.n < 33 || W.n > 16384) return false;
    if (S.kry_ms < 0.0 || W.xprev.last_npos < 0) return false;            // no Lanczos measurement of this block yet
    if (W.xprev.last_npos >= nev) return false;                           // truncation was active last time: the reference's engine decides
    if (S.backoff > 0) { --S.backoff; return false; }                     // after a rejected attempt
    const double est = S.sign_ms >= 0.0 ? S.sign_ms : sign_cost_model_ms(W.nt * dev::TILE);
    if (S.kry_ms < 1.5 * est) { S.streak = 0; return false; }
    if (S.streak >= 256) { S.streak = 0; return false; }                  // re-measure the Lanczos engine now and then
    if (S.disabled) return false;
    const bool inplace = xp == xo;
    if (S.verified_left <= 0) {
        // verification round (first use, then every 64th projection): BOTH engines run on this input; the Lanczos
        // result is the one used, and the engine may serve the next 64 projections only if the two agree.
        // Single-vector Lanczos returns one eigenvector per DISTINCT eigenvalue: where the iterate has repeated
        // positive eigenvalues (MIMO's first iterates) the reference's projection is not the exact one, the
        // comparison fails, and the block stays with the reference's engine for the rest of the solve.
        ShadowBookkeeping keep(*this, idx);
        if (full_eig_by_sign(idx, xp, W.sg_out.p, false, true)) S.check_pending = current_rank[idx] < nev;
        return false;
    }
    double* out = xo;
    if (inplace) {                                                        // keep the input: the check below may reject
        if (W.sg_out.n < (size_t)W.N) W.sg_out.alloc(W.N);
        out = W.sg_out.p;
    }
    const double t0 = now_s();
    if (!full_eig_by_sign(idx, xp, out, fuse, true)) return false;
    const double ms = (now_s() - t0) * 1e3;
    S.sign_ms = S.sign_ms < 0 ? ms : 0.75 * S.sign_ms + 0.25 * ms;
    const int npos = (int)current_rank[idx];
    if (npos >= nev) {                                                    // truncation would be active: not the same projection
        W.lst.sign_engine_rejected++;
        current_rank[idx] = 0;
        S.backoff = 32;
        return false;
    }
    if (inplace) PX_HIP(hipMemcpyAsync(xo, out, (size_t)W.N * sizeof(double), hipMemcpyDeviceToDevice, stream));
    W.lst.sign_engine_projections++;
    S.streak++;
    S.verified_left--;
    min_eig[idx] = 0.0;                 // the reference's value is lambda_min of the returned pairs, <= 0: same decisions
    W.forget_factors();
    return true;
}

// second half of a verification round: xo holds the Lanczos engine's projection, W.sg_out the sign function's
inline void Solver::verify_sign_engine(int idx, const double* xo) {
    EigWork& W = eig[idx];
    W.sign.check_pending = false;
    const bool same = matches_shadow(W, xo);
    W.lst.sign_engine_checks++;
    if (same) {
        W.sign.verified_left = 64;
    } else {
        W.sign.disabled = true;
        W.lst.sign_engine_mismatches++;
    }
}

// full_eig! needs X+ = sum over lambda_i > 0 of lambda_i v_i v_i' -- every POSITIVE eigenpair, not
// the spectrum (prox_operators.jl:115-124), current_rank = #{lambda_i > tol_psd}, min_eig = 0.  The
// reference calls LAPACK dsyevr because it has no partial solver with an unknown count; on this path
// (target_rank beyond max_target_rank_krylov_eigs) the iterate is typically low-rank, so the positive
// part is the top of the spectrum: run the Lanczos engine for g = (positives last time) + slack
// largest pairs; if the smallest of them is <= 0 (and all g converged to krylovkit_tol) every
// positive eigenvalue is among them.  Otherwise enlarge g once, then fall back to the dense solver.
// rocSOLVER dsyevd takes 139 ms at n = 4000 (1.5 TF/s); this takes the cost of a Krylov projection.
inline bool Solver::full_eig_by_lanczos(int idx, const double* xp, double* xo, bool fuse) {
    EigWork& W = eig[idx];
    if (opt.full_eig_lanczos == 0 || opt.eigsolver == 1 || W.n <= opt.min_size_krylov_eigs) return false;
    if (W.xprev.last_npos < 0) return false;                      // no estimate yet: dense eigensolver first
    if (W.fel.disabled) return false;                        // a verification failed earlier in this solve
    // krylovdim = 2 nev + 1 <= cap - 1, and never beyond the step kernels' 255 columns (a wide workspace included)
    const int maxnev = std::min((std::min(W.cap, dev::MAXK - 4) - 2) / 2, W.n - 1);
    int g = W.xprev.last_npos + std::max(3, W.xprev.last_npos / 8);
    if (8 * W.xprev.last_npos > W.n) return false;                // many positive pairs: the dense solver is the cheaper tool
    const bool used_fop = W.use_fop;
    // Verification (options.full_eig_lanczos_verify): this engine is the library's own algorithm, and single-vector
    // Lanczos returns ONE eigenvector per distinct eigenvalue -- a repeated positive eigenvalue, or a start vector
    // deficient in an eigendirection, would silently drop a copy from X+.  On the first call of a block and every
    // k-th after it the reference's engine (full_eig_project: sign function / dsyevd) ALSO projects the same input
    // (into a scratch buffer, BEFORE the reconstruction overwrites an in-place input); the results are compared
    // below and a mismatch hands the block back to the dense engine for the rest of the solve.
    const int vk = opt.full_eig_lanczos_verify < 0 ? 256 : opt.full_eig_lanczos_verify;
    const bool verify = vk > 0 && (W.fel.served % vk) == 0;
    long long ref_rank = 0;
    int ref_npos = 0;
    bool ref_sign = false;
    if (verify) {
        ShadowBookkeeping keep(*this, idx);
        full_eig_project(idx, xp, W.sg_out.p, false);
        ref_rank = current_rank[idx]; ref_npos = W.xprev.last_npos; ref_sign = W.lst.full_eigs_sign > keep.full_eigs_sign;
    }
    auto use_reference_result = [&]() {
        W.fel.disabled = true;
        W.lst.full_eigs_lanczos_mismatches++;
        W.forget_factors(); W.ritz_ok = false;
        if (xp != xo) { full_eig_project(idx, xp, xo, fuse); return; }   // input intact: the ordinary dense call
        // in-place call: the input is gone, the scratch buffer holds the dense engine's projection of it
        PX_HIP(hipMemcpyAsync(xo, W.sg_out.p, (size_t)W.N * sizeof(double), hipMemcpyDeviceToDevice, stream));
        W.lst.full_eigs++;
        if (ref_sign) W.lst.full_eigs_sign++;
        current_rank[idx] = ref_rank; min_eig[idx] = 0.0; W.xprev.last_npos = ref_npos;
    };
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (g > maxnev || g < 1) break;
        lanczos(W, xp, g, true);
        if (!W.converged) {                                   // more positives than g, or no convergence
            if (attempt == 0 && g < maxnev) { g = std::min(2 * g + 2, maxnev); continue; }
            break;
        }
        const int npos = W.count;
        W.fel.served++;
        // guard: between consecutive projections of this regime the number of positive eigenvalues
        // moves by a few; a collapse means the Krylov space was fooled (e.g. decoupled coordinates
        // resolved long before the small positive pairs): let the dense solver decide
        if (npos + 2 + W.xprev.last_npos / 8 < W.xprev.last_npos) break;
        // per-call certificate (Solver::lanczos_certificate): nothing positive may be left outside the returned pairs
        const int cert_m = opt.full_eig_lanczos_certify < 0 ? 10 : opt.full_eig_lanczos_certify;
        if (cert_m >= 2) {
            double theta = 0.0, cscale = 0.0;
            if (lanczos_certificate(W, xp, npos, cert_m, theta, cscale)) {
                const double posres = lanczos_posres();
                if (!(theta <= posres * cscale)) {
                    // a positive direction the run did not see: the dense engine projects this input (intact: the
                    // reconstruction has not run yet); three failures leave the block to the dense engine for good
                    W.lst.full_eigs_lanczos_cert_failed++;
                    if (++W.fel.cert_fails >= 3) W.fel.disabled = true;
                    if (debug) std::fprintf(stderr, "[proxsdp] certificate failed: block %d iteration %lld theta %.3e scale %.3e npos %d\n",
                                            idx, (long long)iter, theta, cscale, npos);
                    break;
                }
                W.lst.full_eigs_lanczos_certified++;
            }
        }
        int rank = 0;
        for (int i = 0; i < npos; ++i) if (W.vals[i] > opt.tol_psd) ++rank;
        // (values are descending: the positive ones are the first npos)
        W.use_fop = false;
        if (used_fop) W.lst.fop_projections++;
        W.lst.full_eigs++; W.lst.full_eigs_lanczos++;
        current_rank[idx] = rank;
        min_eig[idx] = 0.0;                                  // prox_operators.jl:114
        W.xprev.last_npos = npos;
        ritz_pairs_to_block(idx, xp, xo, fuse, 0, npos);
        if (verify) {
            const bool same = matches_shadow(W, xo);
            W.lst.full_eigs_lanczos_checks++;
            if (!same) {
                W.lst.full_eigs--; W.lst.full_eigs_lanczos--;
                use_reference_result();
            }
        }
        return true;
    }
    W.use_fop = false;
    return false;
}

// full_eig! by the dense engines: the sign function where it serves (full_eig_by_sign), else rocSOLVER dsyevd
inline void Solver::full_eig_project(int idx, const double* xp_in, double* xp_out, bool fuse) {
    if (full_eig_by_sign(idx, xp_in, xp_out, fuse)) return;
    EigWork& W = eig[idx];
    std::vector<double> D;
    const bool prof = opt.profile_symv_every > 0;
    if (prof) begin_full_eig_events(W);                   // previous call's events (completed: see the sync below)
    full_eig_values(W, xp_in, dev::INV_SQRT2, true, D);
    if (prof) PX_HIP(hipEventRecord(W.fe[1], stream));
    W.lst.full_eigs++;
    const int n = W.n;
    int npos = 0, rank = 0;
    for (int i = 0; i < n; ++i) { if (D[i] > 0.0) ++npos; if (D[i] > opt.tol_psd) ++rank; }
    current_rank[idx] = rank;
    min_eig[idx] = 0.0;
    W.xprev.last_npos = npos;
    dense_pairs_to_block(idx, xp_in, xp_out, fuse, npos);
    if (prof) { PX_HIP(hipEventRecord(W.fe[2], stream)); W.fe_pending = true; }
}
// The Krylov branch (prox_operators.jl:68-109) for a Krylov dimension the step kernels cannot hold (> 255 columns:
// target_rank > 127, or eigsolver_min_lanczos > 255): the same truncated projection from the dense eigensolver -- the
// top `nev` eigenpairs of dsyevd are what a converged KrylovKit / ARPACK run returns, min_eig is the smallest of them
// (:74,:95), the positive ones among them rebuild the block (:78-85,:99-106).
inline void Solver::truncated_project_dense(int idx, const double* xp_in, double* xp_out, bool fuse, int nev) {
    EigWork& W = eig[idx];
    std::vector<double> D;
    full_eig_values(W, xp_in, dev::INV_SQRT2, true, D);
    const int n = W.n, k = std::min(nev, n);
    int npos = 0;
    for (int i = n - k; i < n; ++i) if (D[i] > 0.0) ++npos;       // ascending: the top k are the trailing k
    min_eig[idx] = D[n - k];
    current_rank[idx] += npos;
    W.xprev.last_npos = npos;
    W.converged = true; W.converged_eigs = k;
    dense_pairs_to_block(idx, xp_in, xp_out, fuse, npos);
    W.forget_factors();
    W.lst.dense_truncated_projections++;
}
// the block from dsyevd's pairs in W.A / W.D (ascending order: the positive eigenpairs are the trailing npos columns)
inline void Solver::dense_pairs_to_block(int idx, const double* xp_in, double* xp_out, bool fuse, int npos) {
    EigWork& W = eig[idx];
    const int n = W.n;
    launch_reconstruct(W, W.A.p + (size_t)(n - npos) * n, n, W.D.p + (n - npos), npos, xp_out,
                       fuse ? xp_in : nullptr, fuse ? idx : -1);
    W.recon_r += npos;
}
// profiled full_eig! (options.profile_symv_every): read the previous call's events, then mark the start of this one
inline void Solver::begin_full_eig_events(EigWork& W) {
    for (Event& e : W.fe) e.create();
    harvest_full_eig_events(W);
    PX_HIP(hipEventRecord(W.fe[0], stream));
}
inline void Solver::harvest_full_eig_events(EigWork& W) {
    if (!W.fe_pending) return;
    W.fe_pending = false;
    if (hipEventSynchronize(W.fe[2]) != hipSuccess) return;
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, W.fe[0], W.fe[1]) == hipSuccess) W.lst.full_eig_solver_ms += a;
    if (hipEventElapsedTime(&b, W.fe[1], W.fe[2]) == hipSuccess) W.lst.full_eig_recon_ms += b;
}

}  // namespace proxsdp
