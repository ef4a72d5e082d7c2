// The host driver of the Lanczos engine (the thick-restart eigsolve behind the PSD projection's Krylov branch), in call order:
// the launches of a step, the rotations, the host logic of a run (parameters, plan, between two cycles, results), the drivers
// (lanczos() and the phases of its cycle, lanczos_eager, lanczos_certificate, lanczos_batch).  Workspace types: solver.hip.hpp.
#pragma once
#include "solver.hip.hpp"

namespace proxsdp {

// a cycle record read back to the host, decoded: alphas | betas | LanczosCtl
struct LzRecord {
    const double* al; const double* be;
    dev::LanczosCtl ctl;
    LzRecord(const double* rec, int ld) : al(rec), be(rec + ld) { std::memcpy(&ctl, rec + 2 * ld, sizeof(ctl)); }
};

// ------------------------------------------------------------------ launches
// launch helper: a profiled launch (`prof` given) carries its own start/stop events (the dispatch's timestamps, i.e. the
// kernel alone, as rocprofv3 reports it -- not the gaps to the neighbouring launches)
template <typename K, typename... Args>
static inline void launch_prof(EigEvents* prof, K kern, dim3 grid, hipStream_t stream, Args... args) {
    if (!prof) { hipLaunchKernelGGL(kern, grid, dim3(dev::TPB), 0, stream, args...); return; }
    const auto e = prof->acquire();
    hipExtLaunchKernelGGL(kern, grid, dim3(dev::TPB), 0, stream, e.first, e.second, 0, args...);
}
// every profile_symv_every-th mat-vec launch of a block is profiled (phase 0: its events are W.ev's), and the
// orthogonalisation behind it (phase 1: W.evo's); null: this launch is not
inline EigEvents* Solver::profiled_launch(EigWork& W, int phase) const {
    if (!(opt.profile_symv_every > 0 && (W.lst.symv_launches % opt.profile_symv_every) == phase)) return nullptr;
    return phase == 0 ? &W.ev : &W.evo;
}

// the operator-form launches of the run in progress are on the owner form (LzPlan::fop_owner): the mat-vec launches write
// W.tred, k_lz_orth reads it.  (lanczos_certificate launches under the plan of the run it certifies: the form's own
// conditions are tested again)
inline bool lz_fop_owner(const EigWork& W) {
    return W.use_fop && W.lzrun.plan.fop_owner && W.pld <= dev::WAVE && W.F_r > 0 && W.F_r <= 2 * W.nt;
}

inline void Solver::launch_symv(EigWork& W, const double* xp, const double* v, bool use_ctl, dev::LanczosCtl* ctl) {
    EigEvents* const prof = profiled_launch(W, 0);
    if (W.use_fop) {
        const bool own = lz_fop_owner(W);
        auto kern = own ? ((W.F_r <= 64) ? dev::k_fop<1, true> : dev::k_fop<2, true>)
                        : ((W.F_r <= 64) ? dev::k_fop<1> : dev::k_fop<2>);
        launch_prof(prof, kern, dim3(own ? 2 * W.nt : W.nt), stream,          // (owner form: nt column owners behind the rows)
                    v, W.prev_factors().V, W.npad, W.F_r,
                    (const int*)W.ell_col.p, (const int*)W.ell_sidx.p, W.ell_w, W.npad, W.esv, W.tpart.p, W.pld,
                    W.ebuf.p, W.apartf.p, (const dev::LanczosCtl*)(use_ctl ? W.ctl_p : nullptr), W.ov, W.tred.p);
    } else {
        launch_prof(prof, dev::k_symv_packed, dim3(W.napart), stream,
                    xp, W.n, W.nt, W.npad, v, W.Ppart.p, (const dev::LanczosCtl*)(use_ctl ? (ctl ? ctl : W.ctl_p) : nullptr), W.Apart.p);
    }
    count_matvecs(W, 1);
}

inline double* lz_hpart(EigWork& W, int k) { return (k & 1) ? W.hpart2.p : W.hpart1.p; }   // partial dots written by the orthogonalisation of step k

// k_symv_finish: closes Lanczos step `kclose` and runs the mat-vec of step kclose+1 on w'
inline void Solver::launch_symv_finish(EigWork& W, const double* xp, int kclose, double tol, bool use_carry) {
    EigEvents* const prof = profiled_launch(W, 0);
    with_nch(kclose + 1, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        if (W.use_fop) {
            const bool own = lz_fop_owner(W);
            auto kern = own ? ((W.F_r <= 64) ? dev::k_fop_finish<1, NCH, true> : dev::k_fop_finish<2, NCH, true>)
                            : ((W.F_r <= 64) ? dev::k_fop_finish<1, NCH> : dev::k_fop_finish<2, NCH>);
            launch_prof(prof, kern, dim3((own ? 3 : 2) * W.nt), stream,
                        (const double*)W.w.p, W.V.p, W.npad, kclose, (const double*)lz_hpart(W, kclose), W.pld,
                        (const double*)W.hsum1.p, W.alphas_p, W.betas_p, W.ctl_p, tol, use_carry ? 1 : 0, W.nt,
                        W.prev_factors().V, W.F_r,
                        (const int*)W.ell_col.p, (const int*)W.ell_sidx.p, W.ell_w, W.npad, W.esv, W.tpart.p,
                        W.ebuf.p, W.apartf.p, W.hred.p, W.ov, W.tred.p);
        } else {
            launch_prof(prof, dev::k_symv_finish<NCH>, dim3(W.nt + W.napart), stream,
                        xp, W.n, W.nt, W.npad, W.Ppart.p, (const double*)W.w.p, W.V.p, W.npad, kclose,
                        (const double*)lz_hpart(W, kclose), W.pld, (const double*)W.hsum1.p, W.alphas_p, W.betas_p, W.ctl_p,
                        tol, use_carry ? 1 : 0, W.Apart.p, W.hred.p);
        }
    });
    count_matvecs(W, 1);
}

// k_lz_finish: closes Lanczos step k (its coefficients land in the record) without a mat-vec behind it
inline void Solver::lz_launch_finish(EigWork& W, int k, double tol, bool use_carry) {
    with_nch(k + 1, [&](auto nch) {
        hipLaunchKernelGGL(dev::k_lz_finish<decltype(nch)::value>, dim3(W.nt), dim3(dev::TPB), 0, stream,
                           (const double*)W.w.p, W.n, W.V.p, W.npad, k, (const double*)lz_hpart(W, k), W.pld,
                           (const double*)W.hsum1.p, W.alphas_p, W.betas_p, W.ctl_p, tol, use_carry ? 1 : 0, W.hred.p);
    });
}

// k_lz_begin: V[:, 0] = the (normalised) start vector, the control block `ctl` cleared
inline void Solver::lz_launch_begin(EigWork& W, const double* start, dev::LanczosCtl* ctl) {
    hipLaunchKernelGGL(dev::k_lz_begin, dim3(ceil_div(W.npad, dev::TPB)), dim3(dev::TPB), 0, stream,
                       W.V.p, start, W.npad, ctl);
}

// k_lz_orth of step k: recurrence, predicted correction and the measured full pass in one launch; the partial-dot buffers
// alternate by step parity (read k - 1, write k).  first: step k opens a cycle (or stands alone: lanczos_eager), its
// couplings with the `keep` columns in front of it are the arrow part at W.arrow_p
inline void Solver::lz_launch_orth(EigWork& W, int k, int first, int keep, EigEvents* prof) {
    dev::FopArgs fo{};
    if (W.use_fop) {
        const EigWork::Factors F = W.prev_factors();
        fo.Vp = F.V; fo.lam = F.lam; fo.rp = F.r;
        fo.tpart = W.tpart.p; fo.tred = W.tred.p; fo.ebuf = W.ebuf.p; fo.apart = W.apartf.p;
    }
    const bool own = lz_fop_owner(W);
    if (own) W.lst.reserved_s[PROXSDP_STATS_FOP_OWNER_STEPS]++;
    auto launch_orth = [&](auto kern) {
        launch_prof(prof, kern, dim3(W.nt), stream,
                    (const double*)W.Ppart.p, W.nt, W.npad, (const double*)W.V.p, W.npad, k, W.w.p,
                    (const double*)W.hred.p, lz_hpart(W, k), W.pld, W.hsum1.p,
                    (const dev::LanczosCtl*)W.ctl_p, (const double*)W.alphas_p, (const double*)W.betas_p,
                    (const double*)W.Apart.p, W.napart, first, (const double*)W.arrow_p, keep, fo);
    };
    with_nch(k + 1, [&](auto nch) {                  // <NCH, NCHP, OWN>: NCHP = 0 packed operator, 1 / 2 operator form (factor rank <= 64 / more)
        constexpr int NCH = decltype(nch)::value;
        if (!W.use_fop) launch_orth(dev::k_lz_orth<NCH, 0>);
        else if (W.F_r <= 64) { if (own) launch_orth(dev::k_lz_orth<NCH, 1, true>); else launch_orth(dev::k_lz_orth<NCH, 1>); }
        else { if (own) launch_orth(dev::k_lz_orth<NCH, 2, true>); else launch_orth(dev::k_lz_orth<NCH, 2>); }
    });
}

// the mat-vec that opens a cycle, on the exact v_k -- or only its count, where the cycle before speculated it into Ppart
inline void Solver::lz_first_matvec(EigWork& W, const double* xp, int k, bool& presymv, dev::LanczosCtl* ctl) {
    if (!presymv) launch_symv(W, xp, W.V.p + (size_t)k * W.npad, true, ctl);
    else count_matvecs(W, 1);
    presymv = false;
}

// the launches of Lanczos step k of a cycle that started at basis column kfirst: the mat-vec (on the exact v_k at the
// start of a cycle, otherwise fused with the closing of step k-1 and run on the uncorrected w') and the
// recurrence / re-orthogonalisation kernel
inline void Solver::lz_launch_step(EigWork& W, const double* xp, int k, int kfirst, double step_tol, bool& presymv) {
    if (k == kfirst) lz_first_matvec(W, xp, k, presymv, W.ctl_p);
    else launch_symv_finish(W, xp, k - 1, step_tol, k - 1 > kfirst);
    lz_launch_orth(W, k, k == kfirst ? 1 : 0, kfirst, profiled_launch(W, 1));
}

// One step of the wide recurrence (lanczos_wide.hip.hpp): mat-vec, two measured Gram-Schmidt passes, closing.
inline void Solver::lzw_step(EigWork& W, LzRun& R, const double* xp, int k) {
    const LzRecBuf& rec = R.plan.rec;
    if (k == R.kfirst) lz_first_matvec(W, xp, k, R.presymv, rec.ctl);
    else launch_symv(W, xp, W.V.p + (size_t)k * W.npad, true, rec.ctl);
    const dev::LanczosCtl* ctl = rec.ctl;
    const int nred = ceil_div(k + 2, dev::TPB);
    hipLaunchKernelGGL(dev::k_lzw_dots, dim3(W.nt), dim3(dev::TPB), 0, stream,
                       (const double*)W.Ppart.p, W.nt, W.npad, (const double*)W.V.p, W.npad, k, W.w.p, W.hpw1.p, ctl);
    hipLaunchKernelGGL(dev::k_lzw_reduce, dim3(nred), dim3(dev::TPB), 0, stream,
                       (const double*)W.hpw1.p, W.pld, W.nt, k, W.hsw1.p, ctl, 0);
    hipLaunchKernelGGL(dev::k_lzw_update, dim3(W.nt), dim3(dev::TPB), 0, stream,
                       W.w.p, (const double*)W.V.p, W.npad, k, (const double*)W.hsw1.p, W.hpw2.p, W.pld, ctl);
    hipLaunchKernelGGL(dev::k_lzw_reduce, dim3(nred), dim3(dev::TPB), 0, stream,
                       (const double*)W.hpw2.p, W.pld, W.nt, k, W.hsw2.p, ctl, 1);
    hipLaunchKernelGGL(dev::k_lzw_close, dim3(W.nt), dim3(dev::TPB), 0, stream,
                       (const double*)W.w.p, W.V.p, W.npad, k, (const double*)W.hsw1.p, (const double*)W.hsw2.p,
                       rec.dev, rec.dev + rec.ld, rec.ctl, R.step_tol);
}

// one-workgroup cycle kernel for medium blocks (lanczos_block1.hip.hpp): the step kernels' arithmetic bit for bit, one launch
// per Lanczos cycle.  lanczos_cycle_kernel: 2 = on, -1 (auto) = on where it applies, 0 = off (1 is read as 0, setup_device).
inline bool Solver::block1_plan(const EigWork& W, int krylovdim, bool split_wanted) const {
    if (!(opt.lanczos_cycle_kernel == 2 || opt.lanczos_cycle_kernel < 0) || block1_lds_cap == 0) return false;
    if (W.nt > dev::B1_MAXNT || krylovdim > dev::B1_KMAX || split_wanted || rot_sink != nullptr) return false;
    // auto: one row group per virtual workgroup (side <= 256).  Measured (profiles/r06_medium_blocks.md): one CU issues ~700
    // instructions per wave and step for 16 waves -- 4.6-5.3 us per step against the step kernels' ~12 at side <= 192 -- but
    // with two row groups per wave (side 257 .. 512) it is 8-12 us per step: no gain, so those sides stay with the step kernels
    if (opt.lanczos_cycle_kernel < 0 && W.nt > dev::B1_NV) return false;
    if (W.use_fop && (W.F_r > 4 * dev::B1_NPV || W.ov.wr_ptr != nullptr || W.ell_w < 1)) return false;
    // the packed triangle must be resident in LDS (one CU cannot stream it from L2 once per step fast enough: measured,
    // profiles/r06_medium_blocks.md); the operator form's E goes there too when it fits, else it is read through L2
    const dev::B1Lds L = dev::b1_lds_plan(W.nt, W.npad, W.use_fop, W.use_fop ? 0 : W.N, 0);
    return (size_t)L.total * sizeof(double) <= (size_t)block1_lds_cap;
}

inline void Solver::launch_block1(EigWork& W, const double* xp, int kfirst, int krylovdim, double tol) {
    dev::Block1Args a{};
    a.xp = xp; a.n = W.n; a.nt = W.nt; a.npad = W.npad;
    a.ldv = W.npad; a.kfirst = kfirst; a.kd = krylovdim; a.tol = tol;
    a.Vout = W.V.p;
    if (W.b1_rot_K > 0) {                        // restart rotation deferred by Solver::rotate: old basis in Z (the pointers were swapped)
        a.Vin = W.Z.p; a.U = W.b1_rot_U; a.rotK = W.b1_rot_K;
        W.b1_rot_K = 0;
    } else {
        a.Vin = W.V.p; a.U = nullptr; a.rotK = 0;
    }
    bool ell_lds = false;
    if (W.use_fop) {
        const EigWork::Factors F = W.prev_factors();
        a.Vp = F.V; a.lam = F.lam; a.rp = F.r;
        a.ell_col = W.ell_col.p; a.ell_sidx = W.ell_sidx.p; a.ell_w = W.ell_w; a.esv = W.esv;
        const dev::B1Lds Le = dev::b1_lds_plan(W.nt, W.npad, true, 0, W.ell_w);
        ell_lds = (size_t)Le.total * sizeof(double) <= (size_t)block1_lds_cap;
    }
    a.ell_in_lds = ell_lds ? 1 : 0;
    W.b1_ell_in_lds = ell_lds;
    a.arrow = W.arrow_p;
    a.alphas = W.alphas_p; a.betas = W.betas_p; a.ctl = W.ctl_p;
    a.dbg = b1_dbg.p;
    const dev::B1Lds L = dev::b1_lds_plan(W.nt, W.npad, W.use_fop, W.use_fop ? 0 : W.N, ell_lds ? W.ell_w : 0);
    const size_t lds = (size_t)L.total * sizeof(double);
    const bool two = W.nt > dev::B1_NV;
    auto kern = W.use_fop ? (two ? dev::k_lz_block1<2, true> : dev::k_lz_block1<1, true>)
                          : (two ? dev::k_lz_block1<2, false> : dev::k_lz_block1<1, false>);
    const bool prof = opt.profile_symv_every > 0;
    if (prof) {
        W.cye[0].create(); W.cye[1].create();
        hipExtLaunchKernelGGL(kern, dim3(1), dim3(dev::B1_TPB), lds, stream, W.cye[0], W.cye[1], 0, a);
        W.cye_pending = true;
    } else {
        hipLaunchKernelGGL(kern, dim3(1), dim3(dev::B1_TPB), lds, stream, a);
    }
    W.lst.cycle_launches++;
    W.lst.cycle_steps += krylovdim - kfirst;
    count_matvecs(W, krylovdim - kfirst);
}

// the cycle record -> `dst` on the host (its pinned mirror rec.host, or an early copy's own), one copy on stream s
inline void Solver::lz_read_record(const LzRecBuf& rec, double* dst, hipStream_t s) {
    PX_HIP(hipMemcpyAsync(dst, rec.dev, rec.doubles * sizeof(double), hipMemcpyDeviceToHost, s));
}

// ------------------------------------------------------------------ rotations
inline void Solver::rotate(EigWork& W, int K, const std::vector<double>& U, int ldu, int ncols,
                           double* out, int copy_src, int copy_dst, const double* extra, int nextra) {
    // U: host column-major (ldu x >=ncols); its K x ncols part goes up compactly, `extra` (the arrow part f | D of the
    // restarted Rayleigh quotient) behind it in the same host-to-device copy: the kernels find it at W.arrow_p
    auto pack = [&](double* dst) {
        for (int c = 0; c < ncols; ++c)
            for (int j = 0; j < K; ++j) dst[(size_t)c * K + j] = U[(size_t)c * ldu + j];
        for (int t = 0; t < nextra; ++t) dst[(size_t)K * std::max(ncols, 0) + t] = extra[t];
    };
    if (rot_sink != nullptr) {
        // batched run: stage the compact K x ncols part (+ the arrow) for ONE upload and ONE launch per cycle
        RotSink::Req& q = rot_sink->slot[W.batch_slot];
        q.W = &W; q.V = W.V.p; q.out = out; q.K = K; q.ncols = ncols; q.copy_src = copy_src; q.copy_dst = copy_dst;
        q.nextra = std::max(nextra, 0); q.valid = true;
        q.data.resize((size_t)K * std::max(ncols, 0) + (size_t)q.nextra);
        pack(q.data.data());
        return;
    }
    // the staging buffer alternates between two slots: two rotations can be in flight between host synchronisations
    // (restart rotation, then the final Ritz-vector one)
    double* tmp = W.Ustage[W.ustage_next].p;
    W.ustage_next ^= 1;
    if ((size_t)K * std::max(ncols, 1) + (size_t)std::max(nextra, 0) > W.ustage_doubles)
        throw std::logic_error("rotation staging buffer too small");
    pack(tmp);
    if (W.lzrun.plan.engine == LzEngine::block1 && nextra > 0 && K < 32 && copy_src == K && copy_dst == ncols && out == W.Z.p) {
        // the next cycle's launch (k_lz_block1) rotates in its prologue, reading U and the arrow part from this pinned buffer
        W.b1_rot_K = K; W.b1_rot_U = tmp;
        W.arrow_p = tmp + (size_t)K * ncols;
        return;
    }
    W.U.upload(tmp, (size_t)K * ncols + (size_t)std::max(nextra, 0), stream);
    if (nextra > 0) W.arrow_p = W.U.p + (size_t)K * ncols;
    rotate_launch(W, K, W.U.p, ncols, out, copy_src, copy_dst);
}

// the launches of rotate(): out[:, :ncols] = V[:, :K] U, U (K x ncols, compact, column-major) on the device
inline void Solver::rotate_launch(EigWork& W, int K, const double* Ud, int ncols, double* out, int copy_src, int copy_dst) {
    W.rot_form = 0; W.rot_launches = 0;
    if (W.lzrun.plan.engine == LzEngine::wide) {         // wide run: LDS-tiled over K (neither form below fits at K > 255)
        if (ncols > 0 || copy_src >= 0) {
            W.rot_form = PROXSDP_ROTATE_WIDE; W.rot_launches = 1;
            hipLaunchKernelGGL(dev::k_lzw_rotate, dim3(W.nt, std::max(1, ceil_div(ncols, dev::LZW_RC))), dim3(dev::TPB), 0, stream,
                               (const double*)W.V.p, W.npad, K, Ud, ncols, out, W.npad, copy_src, copy_dst);
        }
        return;
    }
    // fp64 MFMA form from K = 32 / 16 columns on (skinny GEMM); grid = row tiles x groups of 16 columns; LDS: V tile + one U group
    {
        const int Kp = (K + 3) & ~3;
        const size_t lds_m = ((size_t)Kp * dev::RM_LDV + (size_t)dev::RM_CG * (Kp + 2)) * sizeof(double);
        if (K >= 32 && ncols >= 16 && (int)lds_m <= rotate_mfma_lds_cap) {
            W.rot_form = PROXSDP_ROTATE_MFMA; W.rot_launches = 1;
            hipLaunchKernelGGL(dev::k_lz_rotate_mfma, dim3(W.nt, ceil_div(ncols, dev::RM_CG)), dim3(dev::TPB), lds_m, stream,
                               (const double*)W.V.p, W.npad, K, Ud, ncols, out, W.npad, copy_src, copy_dst);
            return;
        }
    }
    // dynamic LDS: U chunk (K x cn) + V tile (K x 65).  gfx950 has 160 KiB of LDS per CU: the
    // kernel is allowed 144 KiB (setup_device), so a whole restart rotation is ONE launch up to
    // K = 127 (with a 60 KiB cap the V tile alone no longer fitted at K >= 116 and the loop
    // degenerated into one launch per column: 141 launches per iteration at target rank 63)
    const int vbytes = K * (dev::LZ_ROWS + 1) * 8;
    const int maxcols = std::max(1, (rotate_lds_cap - vbytes) / (8 * K));
    int c0 = 0;
    do {
        const int cn = std::max(0, std::min(maxcols, ncols - c0));
        const bool last = (c0 + cn >= ncols);
        if (cn > 0 || (last && copy_src >= 0)) {
            W.rot_form = PROXSDP_ROTATE_SCALAR; W.rot_launches++;
            hipLaunchKernelGGL(dev::k_lz_rotate, dim3(W.nt), dim3(dev::TPB), (size_t)K * cn * 8 + vbytes, stream,
                               W.V.p, W.npad, W.n, K, Ud + (size_t)c0 * K, K, cn,
                               out + (size_t)c0 * W.npad, W.npad, last ? copy_src : -1, copy_dst - c0);
        }
        c0 += std::max(cn, 1);
    } while (c0 < ncols);
}

// the rotations a batched run staged in its sink since the last flush: one upload, one launch (grid.z = block)
inline void Solver::flush_rotations(RotSink& S, BatchCtx& C) {
    dev::LzRotBatch B{};
    size_t used = 0, lds = 0;
    int nt = 0;
    for (RotSink::Req& r : S.slot) {
        if (!r.valid) continue;
        r.valid = false;
        const size_t len = r.data.size();
        if (used + len > (size_t)dev::LZB_MAX * LZB_USTRIDE) throw std::logic_error("flush_rotations: staging buffer too small");
        std::memcpy(C.U_host.p + used, r.data.data(), len * sizeof(double));
        B.r[B.nb++] = dev::LzRot{r.V, C.U.p + used, r.out, r.K, r.ncols, r.copy_src, r.copy_dst};
        if (r.nextra > 0) r.W->arrow_p = C.U.p + used + (size_t)r.K * std::max(r.ncols, 0);
        lds = std::max(lds, ((size_t)r.K * std::max(r.ncols, 0) + (size_t)r.K * (dev::LZ_ROWS + 1)) * sizeof(double));
        B.npad = r.W->npad; nt = r.W->nt;
        used += (len + 7) & ~(size_t)7;
    }
    if (B.nb == 0) return;
    if ((int)lds > rotate_lds_cap) throw std::logic_error("flush_rotations: LDS budget exceeded");
    PX_HIP(hipMemcpyAsync(C.U.p, C.U_host.p, used * sizeof(double), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(dev::k_lzb_rotate, dim3(nt, 1, B.nb), dim3(dev::TPB), lds, stream, B);
}

// ------------------------------------------------------------------ Lanczos (KrylovKit eigsolve)
// Krylov dimension of a positive-part run for nev pairs in a workspace of `cap` columns, krylovdim = krylov_dim(nev)
// (the engine keeps the step kernels' 255 columns in a wide workspace too)
static inline int lz_positive_part_dim(int cap, int krylovdim, int nev, int kdim10) {
    const int mult10 = kdim10 > 0 ? kdim10 : 30;
    return std::min(std::min(cap, dev::MAXK - 4) - 1, std::max(krylovdim, nev * mult10 / 10 + 8));
}

// eigsolver.jl:798-823 -> KrylovKit.eigsolve(A, resid, nev, :LR, Lanczos(orth, krylovdim, maxiter, tol))
// with A = Symmetric(smat(xp)).  eigsolver == 1 selects ARPACK's acceptance rule
// (dsaupd: |resid_i| <= tol*max(eps^(2/3), |theta_i|) for all nev wanted values,
// eigsolver.jl:668-746) on the same thick-restart engine.
// positive_part (full_eig! served by this engine, projection.hip.hpp full_eig_by_lanczos): the wanted
// set is "every eigenpair with lambda > 0", at most nev of them.  A cycle ends the run when all
// positive Ritz pairs are converged to tol AND the first non-positive Ritz pair j is itself resolved
// to 1e-7 of the spectral scale (the solver's own tol_psd is 1e-7; measured on the n = 4000 default
// solve: 1e-9 / 1e-7 / 1e-5 give the same 8643 iterations and the same objective to 1e-13, in
// 21.6 / 18.4 / 12.9 s): a Krylov space that has resolved pair j has (generically) resolved
// everything above it, which is the same reliance every Lanczos acceptance rule makes.  (A residual
// merely smaller than |theta_j| is NOT enough: an unconverged Ritz value is a mixture and can sit
// below zero while small positive eigenvalues are still unresolved -- measured on gpp500-1.)
// Returns the j positive pairs (count = j, possibly 0, converged = true), or converged = false when
// more than nev Ritz values are positive / maxiter is hit.
// parameters of the run and the per-call reset of W; false = the call ends at once (dsaupd argument errors)
inline bool Solver::lz_init(EigWork& W, LzRun& R, int nev, bool positive_part) {
    R.nev = nev; R.positive_part = positive_part;
    // a restart rotation deferred into a launch that never came (an exception in the last run) is void
    W.b1_rot_K = 0; W.b1_rot_U = nullptr;
    R.arpack = (opt.eigsolver == 1);
    int krylovdim = krylov_dim(nev);
    // positive-part mode is the library's own algorithm (not KrylovKit's call): a larger Krylov space
    // resolves the bulk-edge pairs that decide it with fewer restarts (options.full_eig_lanczos_kdim10)
    if (positive_part) krylovdim = lz_positive_part_dim(W.cap, krylovdim, nev, (int)opt.full_eig_lanczos_kdim10);
    if (krylovdim + 1 > W.cap) throw std::invalid_argument("Lanczos workspace too small for the requested rank");
    R.krylovdim = krylovdim;
    if (krylovdim > dev::LZ_KMAX && !W.wide) throw std::logic_error("wide Lanczos: workspace has no wide records");
    R.tol = R.arpack ? opt.arpack_tol : opt.krylovkit_tol;
    R.maxiter = R.arpack ? (long long)opt.arpack_max_iter : (long long)opt.krylovkit_max_iter;
    W.prev_numiter = std::max(W.numiter, 1);
    W.converged = false; W.count = 0; W.converged_eigs = 0; W.numiter = 0; W.vals.clear();
    W.lst.lanczos_calls++;
    if (R.arpack && (!(0 < nev && nev < W.n) || krylovdim > W.n)) return false;   // dsaupd info=-1/-3 -> error -> fallback
    R.step_tol = R.arpack ? 0.0 : R.tol;          // invariant-subspace test inside the recurrence
    R.ld = krylovdim + 1;
    R.T.assign((size_t)R.ld * R.ld, 0.0); R.D.assign(R.ld, 0.0); R.f.assign(R.ld, 0.0);
    R.al.assign(R.ld, 0.0); R.be.assign(R.ld, 0.0);
    R.howmany = nev; R.numiter = 1; R.converged = 0; R.K = 0; R.kfirst = 0; R.pos_count = -1;
    R.pos_fail = false; R.presymv = R.first_speculated = false; R.betaK = 0.0;
    R.split_ready = false; R.merge_active = false;
    R.split_cycle = R.dev_staged = R.merge_on_device = false;
    return true;
}

// The plan of a run, decided once after lz_init.  The engine of the cycles: the wide kernels (Krylov dimension 256..511: never
// the one-workgroup kernel, the operator form, the split eigensolve or a warm start -- all written for at most 255 columns),
// the one-workgroup kernel (medium blocks), or the step kernels.  single_block: the run is lanczos()'s (lanczos_eager's
// mini-cycles and lanczos_batch's batched cycles run on the step kernels and do not split)
inline void Solver::lz_plan(EigWork& W, LzRun& R, bool single_block) {
    LzPlan& p = R.plan;
    const int krylovdim = R.krylovdim;
    const bool wide = krylovdim > dev::LZ_KMAX;
    // split + rank-one merge of the K x K eigensolve (options.host_eig_merge): not for the dsaupd rule (its
    // wanted set is re-ordered afterwards)
    const int merge_from = opt.host_eig_merge == 0 ? (1 << 30) : (opt.host_eig_merge == 1 ? 24 : 64);
    const bool split_wanted = single_block && !R.arpack && krylovdim >= merge_from;
    // one-workgroup cycle kernel (medium blocks): where the split eigensolve would want a mid-cycle read-back the step
    // kernels stay in charge, so that either engine hands the host the same work
    const bool blk1 = single_block && !wide && block1_plan(W, krylovdim, split_wanted);
    p.engine = wide ? LzEngine::wide : blk1 ? LzEngine::block1 : LzEngine::step;
    p.rec = W.record(wide);
    p.split = p.engine == LzEngine::step && split_wanted;
    // the merge itself on the device (options.device_eig_merge): single-block runs of the step kernels on the solver's own
    // thread; a batched run has no split, a block worker thread keeps the host merge (counted as a fallback)
    p.dev_wanted = p.split && (opt.device_eig_merge == 1 || (opt.device_eig_merge < 0 && krylovdim >= 64));
    p.dev_merge = p.dev_wanted && rot_sink == nullptr && StreamRef::tl == nullptr && DeviceMerge::eligible(krylovdim);
    // owner form of the operator-form step (kernels.hip.hpp fop_owner_body): one workgroup per factor column finishes t = Vp'v.
    // Needs the 64 row blocks of a column in one workgroup's registers and a column (or two) per workgroup -- and a column at
    // all (x_prev = 0 off the support has none); lanczos()'s runs only (lanczos_eager runs the packed operator, a batched
    // run the packed kernels)
    p.fop_owner = single_block && fop_owner_knob != 0 && W.use_fop && p.engine == LzEngine::step && W.tred.n > 0 &&
                  W.pld <= dev::WAVE && W.F_r > 0 && W.F_r <= 2 * W.nt;
}

// while the GPU works through the enqueued steps: reduce the arrow part [diag(D) f; f' .] of this cycle's
// Rayleigh quotient (known since the restart) to tridiagonal form, so that only the QL sweep is left on
// the critical path once alpha/beta arrive (host_util.hpp symeig_tridiag_from; K = 53: 108 -> 54 us,
// K = 127: 1330 -> 544 us)
inline void Solver::lz_prepare_arrow(LzRun& R) {
    R.m_arrow = R.kfirst;
    if (R.m_arrow <= 0) return;
    const int n1 = R.m_arrow + 1, ld = R.ld;
    R.Qa.assign((size_t)n1 * n1, 0.0); R.da.assign(n1, 0.0); R.ea.assign(n1, 0.0);
    for (int j = 0; j < R.m_arrow; ++j) {
        R.Qa[(size_t)j * n1 + j] = R.T[(size_t)j * ld + j];
        R.Qa[(size_t)j * n1 + R.m_arrow] = R.Qa[(size_t)R.m_arrow * n1 + j] = R.T[(size_t)j * ld + R.m_arrow];
    }
    householder_tridiag(n1, R.Qa.data(), R.da.data(), R.ea.data());
}

// first phase of the split eigensolve, while the GPU runs the rest of the cycle: wait for the early copy of the
// recurrence coefficients (side stream), decompose T1' = [arrow / first half] - |b| e e'
inline bool Solver::lz_split_first(EigWork& W, LzRun& R) {
    const int k1 = R.k1;
    R.split_ready = false;
    R.m_arrow = 0;                                   // (a failed merge falls back to the dense QL path)
    if (hipEventSynchronize(W.ev_early) != hipSuccess) return false;
    const double t0 = now_s();
    const LzRecord early(W.rec_early.p, R.plan.rec.ld);
    const double* al_e = early.al;
    const double* be_e = early.be;
    const int m = R.kfirst;
    bool ok = !early.ctl.stop;                              // an invariant subspace ends the cycle early: general path
    for (int j = m; ok && j < k1; ++j) ok = (al_e[j] == al_e[j]) && (be_e[j] == be_e[j]) && be_e[j] > 0.0;
    if (ok) {
        std::vector<double> Dk(std::max(m, 1)), fk(std::max(m, 1));
        for (int j = 0; j < m; ++j) { Dk[j] = R.T[(size_t)j * R.ld + j]; fk[j] = R.T[(size_t)j * R.ld + m]; }
        ok = W.split.first(k1, m, Dk.data(), fk.data(), al_e, be_e) == 0;
    }
    R.split_ready = ok;
    // device merge: Q1 goes up on the side stream now, under the remaining steps; the merge's launches wait on its event
    R.dev_staged = false;
    if (ok && R.plan.dev_merge) { W.dmerge.stage_first(W.split, W.side); R.dev_staged = true; }
    W.lst.host_eig_overlap_time += now_s() - t0;
    return ok;
}

// After a cycle's read-back (the record's pinned mirror valid): Rayleigh quotient, K x K eigensolve, convergence.  Returns true
// when the run goes on: the restart rotation has been enqueued and R.kfirst / R.T describe the next cycle;
// false when the run is over (lz_finish_run produces the results).  `speculated`: the first mat-vec of the
// next cycle was already enqueued before the read-back.
inline bool Solver::lz_after_cycle(EigWork& W, LzRun& R, bool speculated) {
    const int krylovdim = R.krylovdim, ld = R.ld, kfirst = R.kfirst, nev = R.nev;
    const double tol = R.tol;
    std::vector<double>& T = R.T; std::vector<double>& D = R.D; std::vector<double>& f = R.f;
    std::vector<double>& al = R.al; std::vector<double>& be = R.be;
    const LzRecord rec(R.plan.rec.host, R.plan.rec.ld);
    std::copy(rec.al, rec.al + krylovdim, al.begin());
    std::copy(rec.be, rec.be + krylovdim, be.begin());
    const int Kend = rec.ctl.stop ? rec.ctl.kstop : krylovdim;
    // launches after the stop flag are no-ops; count the mat-vecs that did work
    W.lst.lanczos_matvecs += (Kend - kfirst);
    count_matvecs(W, -(long long)(krylovdim - Kend));
    W.mv_iter += (Kend - kfirst);
    for (int k = kfirst; k < Kend; ++k) {
        T[(size_t)k * ld + k] = al[k];
        if (k + 1 < Kend) { T[(size_t)k * ld + k + 1] = be[k]; T[(size_t)(k + 1) * ld + k] = be[k]; }
    }
    const int K = R.K = Kend;
    const double betaK = R.betaK = be[K - 1];
    if (!(betaK == betaK)) {                         // NaN guard: treat as not converged
        R.converged = 0; R.pos_fail = true; R.howmany = 0;
        return false;
    }
    if (betaK <= tol && K < R.howmany && !R.arpack) R.howmany = K;
    R.merge_active = false; R.merge_on_device = false;
    if (K > 1 && R.split_ready && K == krylovdim) {
        // split + rank-one merge: T1' was decomposed while the GPU ran the cycle; here the tail and the merge --
        // on the device (merge_device.hip.hpp: D and f come back in one small record, the vectors stay there) or on the host
        const double te0 = now_s();
        double waited = 0.0;                             // (host_eig_time is host compute: not the wait for the record)
        SplitEig& Sp = W.split;
        if (Sp.tail(K, al.data(), be.data()) == 0) {
            bool on_device = false;
            if (R.plan.dev_merge && R.dev_staged)
                on_device = W.dmerge.run(Sp, K, betaK, stream, [&](hipEvent_t e) {
                    const double tw0 = now_s();
                    wait_event(e);
                    waited = now_s() - tw0;
                }, D.data(), f.data());
            if (on_device) {
                W.lst.reserved_s[PROXSDP_STATS_DEVICE_EIG_MERGES]++;
            } else {
                if (R.plan.dev_wanted) W.lst.reserved_s[PROXSDP_STATS_DEVICE_EIG_MERGE_FALLBACKS]++;
                Sp.merge_host();
                R.erow.resize(K);
                Sp.M.row_of_vectors(K - 1, R.erow.data());
                lz_descending(K, Sp.M.evals.data(), R.erow.data(), 1, betaK, D.data(), f.data());
            }
            R.merge_active = true; R.merge_on_device = on_device;
            W.lst.host_eigs++; W.lst.host_eig_merges++;
        }
        W.lst.host_eig_time += now_s() - te0 - waited;
    }
    R.split_ready = false; R.dev_staged = false;
    // (after a merge the Ritz-vector coefficients are formed in lz_restart / lz_finish_run, for the columns actually needed)
    if (!R.merge_active) lz_rayleigh(W, R, K, betaK, true, kfirst == 0);
    int converged = 0;
    if (!R.arpack) {
        // (positive-part mode, the library's own algorithm: optionally a residual RELATIVE to the spectral scale,
        // options.full_eig_lanczos_tol; KrylovKit's rule -- absolute krylovkit_tol -- everywhere else)
        double tol_c = tol;
        if (R.positive_part && opt.full_eig_lanczos_tol > 0.0)
            tol_c = std::max(tol, opt.full_eig_lanczos_tol * std::max(std::fabs(D[0]), std::fabs(D[K - 1])));
        while (converged < K && std::fabs(f[converged]) <= tol_c) ++converged;
    } else {
        const double eps23 = std::pow(2.220446049250313e-16 / 2.0, 2.0 / 3.0);
        int want = std::min(nev, K);
        for (int i = 0; i < want; ++i)
            if (std::fabs(f[i]) <= tol * std::max(eps23, std::fabs(D[i]))) ++converged;
    }
    R.converged = converged;
    if (R.positive_part) {
        int j = 0;
        while (j < K && D[j] > 0.0) ++j;
        if (j > nev) { R.pos_fail = true; return false; }      // more positive pairs than the workspace was sized for
        const double scale = std::max(std::fabs(D[0]), std::fabs(D[K - 1]));
        // the deciding pair: the first STRICTLY negative Ritz value (an exactly-zero pair with zero
        // residual is what a decoupled, unused coordinate of the block looks like: it is found at
        // once and says nothing about the pairs around it)
        int jn = j;
        while (jn < K && D[jn] >= -1e-12 * scale) ++jn;
        const double posres = lanczos_posres();
        if (converged >= j && (jn == K || std::fabs(f[jn]) <= std::max(tol, posres * scale))) { R.pos_count = j; return false; }
        if (K < krylovdim || R.numiter == R.maxiter) { R.pos_fail = true; return false; }
    } else {
        if (converged >= R.howmany) return false;
        if (K < krylovdim) return false;                 // invariant subspace without convergence (arpack rule)
    }
    if (R.numiter == R.maxiter) return false;
    // (positive-part mode, measured in round 4 on the default-options n = 4000 solve, tools/gpurun_r04_pp.sh: Krylov
    // dimension 4g / 5g instead of 3g + 8 and a kept part of positives + 25 % / 40 % of the rest all land within
    // -3 % .. +11 % of this rule's 12.4 s with the same 8651 iterations -- the rule stays)
    const int keep = R.arpack ? std::min(krylovdim - 1, nev + std::max(1, (krylovdim - nev) / 2))
                              : (3 * krylovdim + 2 * converged) / 5;
    lz_restart(W, R, keep, speculated);
    return true;
}

// K x K Rayleigh quotient R.T[:K, :K] -> Ritz values R.D in :LR (descending) order, their vectors R.U and couplings
// R.f = betaK U[K - 1, :].  from_arrow: finish the tridiagonal reduction lz_prepare_arrow started, where it did;
// check_first: symeig_dense's argument
inline void Solver::lz_rayleigh(EigWork& W, LzRun& R, int K, double betaK, bool from_arrow, bool check_first) {
    std::vector<double>& D = R.D; std::vector<double>& U = R.U; std::vector<double>& f = R.f;
    if (K == 1) {
        D[0] = R.T[0]; U.assign(1, 1.0); f[0] = betaK;
        return;
    }
    R.Tw.assign((size_t)K * K, 0.0);
    for (int c = 0; c < K; ++c)
        for (int r = 0; r < K; ++r) R.Tw[(size_t)c * K + r] = R.T[(size_t)c * R.ld + r];
    std::vector<double> Dasc(K);
    const double te0 = now_s();
    if (from_arrow && R.m_arrow > 0 && K > R.m_arrow)
        symeig_tridiag_from(K, R.m_arrow, R.Qa.data(), R.da.data(), R.ea.data(), R.al.data(), R.be.data(), R.Tw.data(), Dasc.data());
    else
        symeig_dense(K, R.Tw.data(), Dasc.data(), check_first);       // (also the fallback of a failed merge: Qa was not prepared)
    W.lst.host_eig_time += now_s() - te0; W.lst.host_eigs++;
    lz_descending(K, Dasc.data(), R.Tw.data() + (K - 1), (size_t)K, betaK, D.data(), f.data());
    U.assign((size_t)K * K, 0.0);
    for (int c = 0; c < K; ++c)
        for (int r = 0; r < K; ++r) U[(size_t)c * K + r] = R.Tw[(size_t)(K - 1 - c) * K + r];
}

// out[:, :ncols] = V[:, :K] U[:, :ncols], U the Ritz-vector coefficients (descending order) of the run's last eigensolve
// wherever they are: on the device after a device merge (no staging, no upload), formed now for these columns after a host
// merge, or R.U.  copy_src, copy_dst, extra, nextra: as rotate() takes them
inline void Solver::lz_rotate_ritz(EigWork& W, LzRun& R, int ncols, double* out, int copy_src, int copy_dst, const double* extra, int nextra) {
    const int K = R.K;
    if (R.merge_on_device) { rotate_launch(W, K, W.dmerge.Uall.p, ncols, out, copy_src, copy_dst); return; }
    if (R.merge_active) {
        const double t0 = now_s();
        std::vector<int> cols(std::max(ncols, 1));
        for (int c = 0; c < ncols; ++c) cols[c] = K - 1 - c;              // evals are ascending
        R.U.assign((size_t)K * std::max(ncols, 1), 0.0);
        if (ncols > 0) W.split.M.vectors(cols.data(), ncols, R.U.data());
        W.lst.host_eig_time += now_s() - t0;
    }
    rotate(W, K, R.U, K, ncols, out, copy_src, copy_dst, extra, nextra);
}

// thick restart on the first `keep` Ritz pairs of the K-column basis: rotation (enqueued), R.T = the arrow [diag(D) f; f' .]
// of the next cycle, which starts at basis column `keep`.  speculated: the mat-vec of v_keep is already under way
inline void Solver::lz_restart(EigWork& W, LzRun& R, int keep, bool speculated) {
    const std::vector<double>& D = R.D; const std::vector<double>& f = R.f;
    // arrow part of the restarted T for k_lz_orth: f (couplings of v_K with the kept Ritz vectors) and D (their Ritz
    // values).  After a device merge its record is f | D in the layout k_lz_orth reads (it stays put until the next
    // merge, a whole cycle away); else it rides behind U.  (The wide kernels measure both passes: no arrow part.)
    const bool arrow = R.plan.engine != LzEngine::wide;
    if (R.merge_on_device) W.arrow_p = W.dmerge.rec_d.p;
    else if (arrow) for (int j = 0; j < keep; ++j) { W.arrow_host.p[j] = f[j]; W.arrow_host.p[dev::MAXK + j] = D[j]; }
    lz_rotate_ritz(W, R, keep, W.Z.p, R.K, keep, W.arrow_host.p, arrow ? 2 * dev::MAXK : 0);   // Z[:, :keep] = V U[:, :keep]; Z[:, keep] = V[:, K]
    std::swap(W.V.p, W.Z.p);
    std::fill(R.T.begin(), R.T.end(), 0.0);
    const int ld = R.ld;
    for (int j = 0; j < keep; ++j) {
        R.T[(size_t)j * ld + j] = D[j];
        R.T[(size_t)j * ld + keep] = f[j];
        R.T[(size_t)keep * ld + j] = f[j];
    }
    R.kfirst = keep;
    R.presymv = R.first_speculated = speculated;
    ++R.numiter;
    W.lst.lanczos_restarts++;
}

// results of the run (KrylovKit's return values / dseupd's), Ritz vectors into W.Z
inline void Solver::lz_finish_run(EigWork& W, LzRun& R) {
    const int K = R.K, nev = R.nev;
    W.numiter = R.numiter;
    if (R.positive_part) {
        if (R.pos_fail || R.pos_count < 0) { W.converged = false; return; }
        W.count = R.pos_count; W.converged_eigs = R.pos_count; W.converged = true;
        W.vals.assign(R.D.begin(), R.D.begin() + R.pos_count);
        if (R.pos_count > 0) lz_rotate_ritz(W, R, R.pos_count, W.Z.p, -1, 0, nullptr, 0);
        return;
    }
    if (R.pos_fail) { W.converged = false; return; }     // NaN guard
    if (R.arpack) {
        // _saupd!/_seupd! (eigsolver.jl:668-746): converged only when all nev pairs are
        W.converged_eigs = R.converged;
        if (R.converged < nev) { W.converged = false; return; }
        W.count = nev;
        W.vals.assign(R.D.begin(), R.D.begin() + nev);
        std::reverse(W.vals.begin(), W.vals.end());      // arc.d is ascending
        std::vector<double> Ur((size_t)K * nev);
        for (int c = 0; c < nev; ++c)
            for (int r = 0; r < K; ++r) Ur[(size_t)c * K + r] = R.U[(size_t)(nev - 1 - c) * K + r];
        rotate(W, K, Ur, K, nev, W.Z.p, -1, 0, nullptr, 0);
        W.converged = true;
        return;
    }
    int howmany = R.howmany;
    if (R.converged > howmany) howmany = R.converged;
    W.count = howmany;
    W.vals.assign(R.D.begin(), R.D.begin() + howmany);
    W.converged_eigs = R.converged;
    W.converged = (R.converged != 0);                    // eigsolver.jl:816-818
    lz_rotate_ritz(W, R, howmany, W.Z.p, -1, 0, nullptr, 0);        // Ritz vectors B*v
}

// ------------------------------------------------------------------ the drivers
// W.resid_host <- the block's Lanczos start vector, normalised: the caller's (`user`, W.n entries) or start_vector's
inline void Solver::lanczos_start_vector(EigWork& W, const double* user) {
    W.resid_host.assign(W.npad, 0.0);
    if (user) std::copy(user, user + W.n, W.resid_host.begin());
    else start_vector(W.n, (uint64_t)opt.eigsolver_resid_seed,
                      opt.eigsolver == 1 ? opt.arpack_resid_init : opt.krylovkit_resid_init,
                      W.resid_host.data());
    double nr = norm2(W.resid_host.data(), W.n);         // KrylovKit: v = x0 / norm(x0)
    if (!(nr > 0.0)) throw std::invalid_argument("Lanczos start vector has zero norm");
    for (int i = 0; i < W.n; ++i) W.resid_host[i] /= nr;
}

// start basis: V[:, 0] normalised and the control block cleared -- from the block's fixed vector (k_lz_begin) or, warm, from the
// previous projection's Ritz vectors.  Warm on the Krylov branch only on request (library-only knob; the reference starts
// every projection from the same fixed vector, krylovkit_reset_resid = false); in positive-part mode (the library's own
// algorithm) by default -- same X+ to krylovkit_tol, fewer restarts (lanczos_warm_start = -1 switches it off there too)
inline void Solver::lz_start_basis(EigWork& W, LzRun& R) {
    const bool warm_start = R.positive_part ? (opt.lanczos_warm_start >= 0) : (opt.lanczos_warm_start > 0);
    if (R.plan.engine == LzEngine::wide || !(warm_start && W.fop_ok && W.have_factors && W.F_r > 0 && W.tpart.n > 0)) {
        lz_launch_begin(W, W.resid.p, R.plan.rec.ctl);
        return;
    }
    const EigWork::Factors F = W.prev_factors();
    const int nb = ceil_div(W.npad, dev::TPB);
    hipLaunchKernelGGL(dev::k_lz_warm_sum, dim3(nb), dim3(dev::TPB), 0, stream,
                       W.V.p, F.V, W.npad, F.r, (const double*)W.resid.p, W.npad, W.warm_part.p,
                       (const double*)(R.positive_part && F.r <= dev::TPB ? F.lam : nullptr),
                       R.positive_part ? opt.full_eig_lanczos_warm_pow : 0.0);
    hipLaunchKernelGGL(dev::k_lz_warm_scale, dim3(nb), dim3(dev::TPB), 0, stream,
                       W.V.p, W.npad, (const double*)W.warm_part.p, nb, W.ctl_p);
    W.lst.warm_starts++;
}

// arm the split of a run whose plan asks for it: the merge's helper threads spin while `helpers` lives (not from a block
// worker thread: one pool per solver); side stream, events and the early record's mirror on first use
inline void Solver::lz_arm_split(EigWork& W, LzRun& R, ArmedPool& helpers) {
    W.split.M.par = nullptr;
    if (!R.plan.split) return;
    if (merge_helpers() > 0 && StreamRef::tl == nullptr) {
        if (!merge_pool) {
            merge_pool.reset(new SpinPool(merge_helpers()));
            merge_par = [this](int n, const std::function<void(int)>& body) { merge_pool->run(n, body); };
        }
        helpers.arm(merge_pool.get());
        W.split.M.par = &merge_par;
        W.split.M.nchunk = merge_helpers() + 1;
    }
    if (W.side == nullptr) {
        W.side.create(hipStreamNonBlocking);
        W.ev_mid.create(hipEventDisableTiming);
        W.ev_early.create(hipEventDisableTiming);
        W.rec_early.alloc(R.plan.rec.doubles);
    }
}

// enqueue the cycle's steps kfirst .. krylovdim - 1 on the run's engine; step engine, split cycle: once the launch of step k1
// has closed step k1 - 1, the record goes out on the side stream while the cycle runs on
inline void Solver::lz_enqueue_cycle(EigWork& W, LzRun& R, const double* xp) {
    const int kfirst = R.kfirst, krylovdim = R.krylovdim;
    switch (R.plan.engine) {
    case LzEngine::wide:
        for (int k = kfirst; k < krylovdim; ++k) lzw_step(W, R, xp, k);
        break;
    case LzEngine::block1:
        launch_block1(W, xp, kfirst, krylovdim, R.step_tol);
        R.presymv = false;
        break;
    case LzEngine::step:
        for (int k = kfirst; k < krylovdim; ++k) {
            lz_launch_step(W, xp, k, kfirst, R.step_tol, R.presymv);
            if (R.split_cycle && k == R.k1) {
                PX_HIP(hipEventRecord(W.ev_mid, stream));
                PX_HIP(hipStreamWaitEvent(W.side, W.ev_mid, 0));
                lz_read_record(R.plan.rec, W.rec_early.p, W.side);
                PX_HIP(hipEventRecord(W.ev_early, W.side));
            }
        }
        lz_launch_finish(W, krylovdim - 1, R.step_tol, krylovdim - 1 > kfirst);
        break;
    }
}

// speculate: the first mat-vec of a possible next cycle needs only v_K = V[:, krylovdim], final now -- enqueued before the host
// round trip (wasted only when this cycle is the last), and only when this block's previous projection restarted too
inline bool Solver::lz_speculate(EigWork& W, LzRun& R, const double* xp) {
    if (R.plan.engine == LzEngine::block1 || !(W.prev_numiter > 1 || R.numiter > 1)) return false;
    launch_symv(W, xp, W.V.p + (size_t)R.krylovdim * W.npad, true, R.plan.rec.ctl);
    count_matvecs(W, -1);                             // counted when used
    return true;
}

// read back: the record's copy, the host work under the GPU's cycle (first part of the split eigensolve, or the arrow
// reduction of the QL path), the wait, the harvest of the cycle's profile events
inline void Solver::lz_read_back(EigWork& W, LzRun& R) {
    lz_read_record(R.plan.rec, R.plan.rec.host, stream);
    if (!(R.split_cycle && lz_split_first(W, R))) lz_prepare_arrow(R);
    const double t0 = debug ? now_s() : 0.0;
    wait_stream();
    if (debug) { dbg_lz.wait += now_s() - t0; dbg_lz.cycles += 1.0; }
    if (W.cye_pending) {
        W.cye_pending = false;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, W.cye[0], W.cye[1]) == hipSuccess) W.lst.cycle_ms += ms;
    }
    W.ev.harvest(W.lst.symv_profiled_ms, W.lst.symv_profiled);
    W.evo.harvest(W.lst.orth_profiled_ms, W.lst.orth_profiled);
}

inline void Solver::lanczos(EigWork& W, const double* xp, int nev, bool positive_part) {
    W.ritz_ok = false;                                   // Z / vals are about to be rewritten
    if (opt.krylovkit_eager && opt.eigsolver != 1 && !positive_part) { lanczos_eager(W, xp, nev); return; }
    LzRun& R = W.lzrun;
    if (!lz_init(W, R, nev, positive_part)) return;
    lz_plan(W, R, true);
    const int krylovdim = R.krylovdim;
    if (R.plan.engine == LzEngine::wide) W.lst.wide_krylov_projections++;
    if (krylovdim >= 96) QlPool::get().arm();            // host eigensolve helpers wake up under the first Lanczos cycle
    lz_start_basis(W, R);
    ArmedPool merge_helpers_armed;
    lz_arm_split(W, R, merge_helpers_armed);
    while (true) {
        // split point: the arrow with its hub after a restart, the first half of the tridiagonal in the first cycle;
        // the coefficients of step k1 - 1 exist once the launch of step k1 has closed it
        // (first cycle: T1 takes 72 % of the steps -- its QL, ~0.45 ms (k1/127)^3, still ends before the remaining
        // steps do, and the tail left for the critical path shrinks to a quarter of the basis: (0.28)^3 of the QL work)
        R.k1 = (R.kfirst == 0) ? (18 * krylovdim) / 25 : R.kfirst + 1;
        R.split_cycle = R.plan.split && R.k1 >= 1 && R.k1 <= krylovdim - 2;
        lz_enqueue_cycle(W, R, xp);
        const bool speculated = lz_speculate(W, R, xp);
        lz_read_back(W, R);
        if (lz_observer) (*lz_observer)(W, R);
        const double t1 = debug ? now_s() : 0.0;
        const bool go_on = lz_after_cycle(W, R, speculated);
        if (debug) dbg_lz.after_cycle += now_s() - t1;
        if (!go_on) break;
    }
    const double t2 = debug ? now_s() : 0.0;
    lz_finish_run(W, R);
    if (debug) dbg_lz.results += now_s() - t2;
}

// KrylovKit's `eager = true` (options.jl:112, eigsolver.jl:809): the Rayleigh quotient is decomposed and the convergence
// test made after EVERY expansion step once the basis holds `howmany` vectors, not only when it is full -- a projection
// ends as soon as its wanted pairs have converged.  Off by default in the reference; here every such step is a
// mini-cycle of the same kernels: mat-vec on the exact v_k, recurrence + full re-orthogonalisation (`first` form of
// k_lz_orth with the coupling beta_{k-1} e_{k-1} as its "arrow"), step closing, read-back, K x K eigensolve on the
// host.  Three launches and one synchronisation per step: a faithful, not a fast, mode.  Packed-triangle operator.
inline void Solver::lanczos_eager(EigWork& W, const double* xp, int nev) {
    LzRun& R = W.lzrun;
    W.use_fop = false;
    if (!lz_init(W, R, nev, false)) return;
    lz_plan(W, R, false);
    if (R.arpack) throw std::invalid_argument("krylovkit_eager applies to eigsolver = 2 (KrylovKit) only");
    if (R.plan.engine == LzEngine::wide) throw std::invalid_argument("krylovkit_eager: Krylov dimension > 255 is not supported");
    const int kd = R.krylovdim, ld = R.ld;
    const double tol = R.tol;
    lz_launch_begin(W, W.resid.p, W.ctl_p);
    std::vector<double>& T = R.T; std::vector<double>& f = R.f;
    std::vector<double> fstep(2 * dev::MAXK, 0.0);
    int K = 0, kfirst = 0, converged = 0;
    double beta = 0.0;
    while (true) {
        const int k = K;                                  // expand: v_k is an exact, normalised basis vector
        launch_symv(W, xp, W.V.p + (size_t)k * W.npad, true);
        int keep = kfirst;
        if (k > kfirst) {                                 // ordinary step: w -= beta_{k-1} v_{k-1}
            std::fill(fstep.begin(), fstep.begin() + k, 0.0);
            fstep[k - 1] = beta;
            W.arrow.upload(fstep.data(), (size_t)k, stream);
            W.arrow_p = W.arrow.p;
            keep = k;
        }
        lz_launch_orth(W, k, 1, keep, nullptr);
        lz_launch_finish(W, k, 0.0, false);
        lz_read_record(R.plan.rec, R.plan.rec.host, stream);
        PX_HIP(hipStreamSynchronize(stream));
        const LzRecord rec(R.plan.rec.host, R.plan.rec.ld);
        const double al_k = rec.al[k];
        beta = rec.be[k];
        W.lst.lanczos_matvecs++; W.mv_iter++;
        if (!(beta == beta) || !(al_k == al_k)) { R.pos_fail = true; R.K = K; break; }      // NaN guard
        T[(size_t)k * ld + k] = al_k;
        if (k > kfirst) { T[(size_t)(k - 1) * ld + k] = T[(size_t)k * ld + (k - 1)] = rec.be[k - 1]; }
        K = k + 1;
        if (beta <= tol && K < R.howmany) R.howmany = K;
        if (K == kd || beta <= tol || K >= R.howmany) {
            lz_rayleigh(W, R, K, beta, false, false);
            converged = 0;
            while (converged < K && std::fabs(f[converged]) <= tol) ++converged;
            R.K = K; R.converged = converged;
            if (converged >= R.howmany) break;
        }
        if (K < kd) {
            if (beta <= tol) { R.K = K; break; }          // invariant subspace (howmany was reduced above: not reached normally)
            continue;
        }
        if (R.numiter == R.maxiter) break;
        lz_restart(W, R, (3 * kd + 2 * converged) / 5, false);
        kfirst = K = R.kfirst;
    }
    lz_finish_run(W, R);
}

// Certificate of a Lanczos-served full_eig! (options.full_eig_lanczos_certify).  Single-vector Lanczos
// returns one eigenvector per DISTINCT eigenvalue the start vector has a component along: a repeated positive eigenvalue or
// a deficient start vector silently drops positive eigenpairs from X+.  After the run has converged with npos positive
// pairs (Ritz vectors in W.Z, values in W.vals) a SECOND, independent pseudo-random vector is orthogonalised against them
// and run through `msteps` steps of the same recurrence with the Ritz vectors as the locked part of the basis (a thick
// restart whose coupling row is zero): Lanczos on the operator deflated by the returned pairs.  Everything that is left
// must be <= 0; the largest Ritz value of the msteps x msteps tridiagonal is a LOWER bound of the largest remaining
// eigenvalue and converges to an isolated one within a few steps.  Returns false when the check could not run (workspace
// too small, non-finite coefficients); theta_max / scale are what the caller tests.
// What ten steps of the plain fp64 recurrence give (NumPy, tests/positive_part_cases.py certificate_reference; sides 130, 257,
// 520, 0 .. 100 locked pairs 9 .. 1, the rest in [-3, -0.5], 5 seeds): theta_max in [-0.61, -0.50] when nothing positive is left;
// 7.000 to four digits with one eigenvalue 7 outside the locked pairs; anywhere in [-0.11, 1e-3] with one at 1e-3 -- ten steps do
// not promise to find a small isolated positive value (the device's values: profiles/positive_part.md; the kernels of this
// function against that recurrence: tests/test_positive_part.py).
inline bool Solver::lanczos_certificate(EigWork& W, const double* xp, int npos, int msteps, double& theta_max, double& scale) {
    if (npos + msteps + 1 > W.cap || npos + msteps + 1 > dev::KLD || msteps < 2) return false;
    if (W.resid2.n == 0) {
        std::vector<double> r2(W.npad, 0.0);
        start_vector(W.n, (uint64_t)opt.eigsolver_resid_seed ^ 0x9e3779b97f4a7c15ull, 3, r2.data());   // (normalised)
        W.resid2.alloc(W.npad);
        W.resid2.upload(r2.data(), W.npad, stream);
        PX_HIP(hipStreamSynchronize(stream));                       // (r2 goes out of scope)
    }
    std::swap(W.V.p, W.Z.p);                                        // the basis buffer holds the Ritz vectors in columns [0, npos)
    if (npos == 0) {
        lz_launch_begin(W, W.resid2.p, W.ctl_p);
    } else {
        // v_npos = (r - Z Z'r) / |.|: measured dots, then the ordinary step closing
        PX_HIP(hipMemcpyAsync(W.w.p, W.resid2.p, (size_t)W.npad * sizeof(double), hipMemcpyDeviceToDevice, stream));
        const int kc = npos - 1;
        with_nch(npos, [&](auto nch) {
            hipLaunchKernelGGL(dev::k_lz_measure<decltype(nch)::value>, dim3(W.nt), dim3(dev::TPB), 0, stream,
                               (const double*)W.w.p, (const double*)W.V.p, W.npad, kc, lz_hpart(W, kc), W.pld, W.ctl_p);
        });
        lz_launch_finish(W, kc, 0.0, false);
    }
    // locked part: coupling row f = 0, Ritz values D (the prediction of k_lz_orth multiplies the measured junk by them)
    for (int j = 0; j < npos; ++j) { W.arrow_host.p[j] = 0.0; W.arrow_host.p[dev::MAXK + j] = W.vals[j]; }
    if (npos > 0) {
        PX_HIP(hipMemcpyAsync(W.arrow.p, W.arrow_host.p, (size_t)npos * sizeof(double), hipMemcpyHostToDevice, stream));
        PX_HIP(hipMemcpyAsync(W.arrow.p + dev::MAXK, W.arrow_host.p + dev::MAXK, (size_t)npos * sizeof(double), hipMemcpyHostToDevice, stream));
    }
    W.arrow_p = W.arrow.p;
    const int kend = npos + msteps;
    bool presymv = false;
    for (int k = npos; k < kend; ++k) lz_launch_step(W, xp, k, npos, 0.0, presymv);
    lz_launch_finish(W, kend - 1, 0.0, kend - 1 > npos);
    const LzRecBuf narrow = W.record(false);
    lz_read_record(narrow, narrow.host, stream);
    wait_stream();
    std::swap(W.V.p, W.Z.p);
    W.evo.used = 0; W.ev.used = 0;                                  // (profile events recorded by lz_launch_step: not a projection's)
    W.lst.lanczos_matvecs += msteps; W.mv_iter += msteps; W.lst.cert_matvecs += msteps;
    // the deflated recurrence may end early (beta <= 0 exactly: what is left of the operator acts as a multiple of the
    // identity on the complement -- the later launches are no-ops and their record entries are stale values of the main
    // run): only the steps that ran form the tridiagonal
    const LzRecord rec(narrow.host, narrow.ld);
    if (rec.ctl.stop) msteps = std::max(0, std::min(msteps, rec.ctl.kstop - npos));
    if (msteps < 1) return false;
    const double* al = rec.al + npos;
    const double* be = rec.be + npos;
    std::vector<double> T((size_t)msteps * msteps, 0.0), d(msteps, 0.0);
    for (int j = 0; j < msteps; ++j) {
        if (!(al[j] == al[j]) || !(j + 1 < msteps ? be[j] == be[j] : true)) return false;
        T[(size_t)j * msteps + j] = al[j];
        if (j + 1 < msteps) T[(size_t)j * msteps + j + 1] = T[(size_t)(j + 1) * msteps + j] = be[j];
    }
    if (msteps == 1) d[0] = al[0];
    else if (symeig_dense(msteps, T.data(), d.data(), true) != 0) return false;
    theta_max = d[msteps - 1];
    scale = std::max({std::fabs(d[0]), std::fabs(theta_max), npos > 0 ? std::fabs(W.vals[0]) : 0.0});
    return true;
}

// KrylovKit eigsolve of SEVERAL blocks of equal side at once (kernels.hip.hpp "BATCHED Lanczos step"): one
// launch per step for all of them (grid.z = block) on the solver's stream, per-block host restart logic
// (lz_after_cycle) between the cycles.  Per block the arithmetic, the mat-vec count and the restart count are
// those of lanczos(); blocks that have converged drop out of the launches.  Preconditions (checked by
// batch_eligible): plain KrylovKit mode, packed-triangle operator, krylovdim <= 63.
inline void Solver::lanczos_batch(const std::vector<int>& blocks, const double* xbase, const std::vector<int>& nevs, int ctx_slot) {
    const int nb = (int)blocks.size();
    if (ctx_slot < 0 || ctx_slot >= (int)batch_ctx.size() || !batch_ctx[ctx_slot]) throw std::logic_error("lanczos_batch: no context for this group");
    BatchCtx& C = *batch_ctx[ctx_slot];
    const bool concurrent = StreamRef::tl != nullptr;        // running on a group worker thread: shared counters go through a lock
    long long steps_local = 0;
    if (nb < 1 || nb > dev::LZB_MAX) throw std::invalid_argument("lanczos_batch: 1..LZB_MAX blocks");
    auto Rq = [&](int q) -> LzRun& { return eig[blocks[q]].lzrun; };     // host state of block q's run (lives in its workspace)
    std::vector<char> live(nb, 0), ran(nb, 0);
    EigWork& W0 = eig[blocks[0]];
    dev::LzBatch B{};
    B.n = W0.n; B.nt = W0.nt; B.npad = W0.npad; B.pld = W0.pld; B.napart = W0.napart; B.nb = nb;
    for (int q = 0; q < nb; ++q) {
        EigWork& W = eig[blocks[q]];
        W.use_fop = false;
        W.ritz_ok = false;
        W.batch_slot = q;
        live[q] = ran[q] = lz_init(W, Rq(q), nevs[q], false) ? 1 : 0;
        lz_plan(W, Rq(q), false);
        if (Rq(q).krylovdim > 63) throw std::invalid_argument("lanczos_batch: krylovdim > 63");
        B.tol = Rq(q).step_tol;
    }
    auto fill = [&](int q) -> dev::LzBlk& {
        EigWork& W = eig[blocks[q]];
        dev::LzBlk& b = B.b[q];
        b.xp = xbase + P.blocks[blocks[q]].off;
        b.Ppart = W.Ppart.p; b.wbuf = W.w.p; b.V = W.V.p; b.hpart1 = W.hpart1.p; b.hpart2 = W.hpart2.p;
        b.hsum = W.hsum1.p; b.alphas = W.alphas_p; b.betas = W.betas_p; b.ctl = W.ctl_p; b.Apart = W.Apart.p;
        b.hred = W.hred.p; b.arrow = W.arrow_p; b.resid = W.resid.p;
        return b;
    };
    const int ntile = W0.napart;
    if (C.U.n == 0) {
        C.U.alloc(dev::LZB_MAX * LZB_USTRIDE); C.U_host.alloc(dev::LZB_MAX * LZB_USTRIDE);
        C.rec_host.alloc(dev::LZB_MAX * EigWork::REC_DOUBLES);
    }
    RotSink sink;
    // helper threads for the restart logic (options.block_threads: -1 auto = one per block up to 8, 0 = none): they spin
    // only while this projection is in progress
    const int nhelp = std::min(nb, opt.block_threads < 0 ? 8 : (int)opt.block_threads) - 1;
    if (nhelp >= 1 && (!C.pool || C.pool->helpers() < nhelp)) C.pool.reset(new SpinPool(nhelp));
    SpinPool* pool = (nhelp >= 1) ? C.pool.get() : nullptr;
    struct SinkGuard {                                   // the sink installed and the helpers spinning while the run lasts
        ArmedPool helpers;
        SinkGuard(RotSink* s, SpinPool* p) : helpers(p) { Solver::rot_sink = s; }
        ~SinkGuard() { Solver::rot_sink = nullptr; }
    } guard(&sink, pool);
    for (int q = 0; q < nb; ++q) fill(q).mode = live[q] ? 1 : 0;
    hipLaunchKernelGGL(dev::k_lzb_begin, dim3(ceil_div(W0.npad, dev::TPB), 1, nb), dim3(dev::TPB), 0, stream, B);
    long long nlaunch = 0, prof_blocks = 0;
    double tp0 = debug ? now_s() : 0.0;                  // PROXSDP_HIP_DEBUG: host-time split of the batched run
    auto lap = [&](double& acc) { if (debug && !concurrent) { const double t = now_s(); acc += t - tp0; tp0 = t; } };
    std::vector<char> presymv(nb, 0);                // the first mat-vec of the block's next cycle is already in Ppart (speculated)
    C.ev.create(hipEventDisableTiming);
    double* const rec_out = C.rec_host.p;
    const int rec_n = (int)EigWork::REC_DOUBLES;
    while (true) {
        int tmax = 0, nlive = 0;
        for (int q = 0; q < nb; ++q)
            if (live[q]) { tmax = std::max(tmax, Rq(q).krylovdim - Rq(q).kfirst); ++nlive; }
        if (nlive == 0) break;
        for (int t = 0; t <= tmax; ++t) {
            bool any_orth = false, any_mv = false;
            for (int q = 0; q < nb; ++q) {
                dev::LzBlk& b = fill(q);               // (V / arrow pointers change at a restart)
                b.mode = 0;
                if (!live[q]) continue;
                const int k = Rq(q).kfirst + t, kd = Rq(q).krylovdim;
                b.k = k; b.keep = Rq(q).kfirst;
                b.mode = (t == 0) ? (presymv[q] ? 0 : 1) : (k < kd) ? 2 : (k == kd) ? 3 : 0;
                any_mv = any_mv || b.mode != 0;
                if (k < kd) {
                    any_orth = true;
                    count_matvecs(eig[blocks[q]], 1);
                }
            }
            // every profile_symv_every-th batched mat-vec launch carries its own start/stop events
            const bool prof = any_mv && opt.profile_symv_every > 0 && t > 0 && t < tmax && (nlaunch++ % opt.profile_symv_every) == 0;
            if (any_mv)                 // (t = 0 with every live block's first mat-vec already speculated: nothing to launch)
                launch_prof(prof ? &W0.ev : nullptr, dev::k_lzb_mv, dim3(W0.nt + ntile, 1, nb), stream, B, rec_out, rec_n);
            for (int q = 0; prof && q < nb; ++q) prof_blocks += (B.b[q].mode == 2) ? 1 : 0;
            if (!any_orth) continue;
            for (int q = 0; q < nb; ++q) {
                dev::LzBlk& b = B.b[q];
                const bool act = live[q] && b.k < Rq(q).krylovdim;       // step b.k of the block's cycle exists
                b.mode = act ? 1 : 0;                                     // (k_lzb_orth: != 0 = active)
            }
            hipLaunchKernelGGL(dev::k_lzb_orth, dim3(W0.nt, 1, nb), dim3(dev::TPB), 0, stream, B);
            steps_local += nlive;
        }
        // every live block's record [alphas | betas | ctl] has been copied out by the closing workgroup 0 of its mode-3 launch
        // (straight into pinned host memory): the host waits for THAT point of the stream ...
        PX_HIP(hipEventRecord(C.ev, stream));
        // ... while the GPU already runs the first mat-vec of every block's NEXT cycle (on v_K = V[:, krylovdim], final since
        // the mode-3 closing; the restart rotation copies it to column `keep`, so the tiles' result stays valid) -- wasted
        // only for the blocks that turn out to have converged
        for (int q = 0; q < nb; ++q) {
            dev::LzBlk& b = fill(q);
            b.mode = live[q] ? 1 : 0;
            b.k = live[q] ? Rq(q).krylovdim : 0; b.keep = 0;
        }
        hipLaunchKernelGGL(dev::k_lzb_mv, dim3(W0.nt + ntile, 1, nb), dim3(dev::TPB), 0, stream, B, (double*)nullptr, 0);
        for (int q = 0; q < nb; ++q) presymv[q] = live[q];
        for (int q = 0; q < nb; ++q) if (live[q]) lz_prepare_arrow(Rq(q));
        lap(dbg_batch.enqueue);                          // (+ arrow reductions)
        wait_event(C.ev);
        lap(dbg_batch.wait);
        for (int q = 0; q < nb; ++q)
            if (live[q]) std::memcpy(eig[blocks[q]].rec_host, C.rec_host.p + (size_t)q * EigWork::REC_DOUBLES, EigWork::REC_DOUBLES * sizeof(double));
        W0.ev.harvest(W0.lst.symv_profiled_ms, W0.lst.symv_profiled);
        // per-block restart logic (K x K eigensolve, convergence, rotation matrix): independent, on the helper threads
        std::exception_ptr err[dev::LZB_MAX] = {};
        auto job = [&](int q) {
            if (!live[q]) return;
            RotSink* const prev = Solver::rot_sink;          // (thread-local: a helper thread stages into THIS run's sink)
            Solver::rot_sink = &sink;
            try { live[q] = lz_after_cycle(eig[blocks[q]], Rq(q), false) ? 1 : 0; }
            catch (...) { err[q] = std::current_exception(); live[q] = 0; }
            Solver::rot_sink = prev;
        };
        if (pool) pool->run(nb, job);
        else for (int q = 0; q < nb; ++q) job(q);
        for (int q = 0; q < nb; ++q) if (err[q]) std::rethrow_exception(err[q]);
        lap(dbg_batch.restart);
        flush_rotations(sink, C);                    // the restart rotations of this cycle: one upload, one launch
        lap(dbg_batch.flush);
        if (!concurrent) dbg_batch.cycles += 1.0;
    }
    for (int q = 0; q < nb; ++q) if (ran[q]) lz_finish_run(eig[blocks[q]], Rq(q));
    flush_rotations(sink, C);                        // the Ritz vectors of every block
    {
        std::lock_guard<std::mutex> lk(batch_stats_mu);
        st.batched_block_steps += steps_local;
        st.batched_profiled_blocks += prof_blocks;   // blocks served by the event-bracketed launches (bytes = this x (8N + 16n))
    }
}

}  // namespace proxsdp
