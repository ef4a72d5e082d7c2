// A model that stays set up on the device between solves (include/proxsdp_hip.h "model handle"): one live Solver on storage
// of its own, the index maps its data is replaced through (model_update.hip.hpp), and the counters proxsdp_hip_model_info
// reports.  No line of the reference stands behind this file: ProxSDP builds AffineSets, ConicSets, the operator and every
// workspace anew in each optimize! (/root/reference/src/MOI_wrapper.jl:220-342).
//
// create  = everything Solver::run does before initial_steps() (Solver::setup) + the device exit path's set-up, once
// solve   = Solver::reset_for_solve() + Solver::solve(): proxsdp_hip_solve_device on the model's current data, bit for bit
// update  = the caller's new numbers through the recorded maps into the device arrays, the four norms, and -- when the zero
//           pattern of c moved the support set -- setup_support() / alloc_candidates() once more
// rows    = inequality rows added and dropped (model_rows.hip.hpp): a second RowState (solver.hip.hpp: every buffer sized by Q,
//           nnz or the pattern) built for the new shape, filled from the live one through the plan's source maps, and exchanged
//           with it; everything sized by n or a cone side stays
// The tools read the handle and write nothing of it; their scratch is the call's own (bytes_allocated, not device_bytes):
// triangles, cliques = the violated triangle rows of a cone, and given bases grown by two nodes (triangle_cuts.hip.hpp,
//           clique_cuts.hip.hpp): read the cone's variable list
// inactive_rows = the inequality rows that went slack (triangle_cuts.hip.hpp): reads m
// round   = a +-1 vector from a cone's factors against the current c (rounding.hip.hpp): reads the exit path's c
// bound   = a certified lower bound of the optimum from any dual point (dual_bound.hip.hpp): reads the exit path's c, values
//           and [b; h] and the host mirror of the rows
// The entry points (argument checks, error codes) are in capi.hip; what a call needs round its kernels is model_call.hip.hpp.
#pragma once
#include "model_call.hip.hpp"
#include "model_update.hip.hpp"
#include "model_rows.hip.hpp"
#include "triangle_cuts.hip.hpp"
#include "clique_cuts.hip.hpp"
#include "rounding.hip.hpp"
#include "dual_bound.hip.hpp"

struct proxsdp_model {
    std::atomic<long long> bytes{0};            // live device bytes (DevAccount); first member: outlives every buffer below
    proxsdp_options opt0{};                     // create's options, as given
    proxsdp_result scratch{};                   // the result the solver writes: rebound to the caller's arrays per solve
    std::vector<double> resid;                  // copy of proxsdp_problem.eig_resid
    std::vector<int64_t> psd_ptr;               // the cone lists' offsets, for the argument checks of a solve
    proxsdp_problem shape{};                    // n, p, m, n_psd, psd_ptr: what those checks read of a problem
    int64_t solves = 0, updates = 0, support_rebuilds = 0;
    double setup_time = 0.0;
    int index_base = 0;                         // of create: the columns of added rows follow it
    std::unique_ptr<proxsdp::Solver> S;
    proxsdp::DevBuf<int> sinv_d, flag_d;
    proxsdp::DevBuf<long long> ord_d;
    proxsdp::DevBuf<double> stage, npart, nout;

    // device allocations of this thread (and of the block workers started under it) count for this model while one lives
    struct Accounting {
        std::atomic<long long>* prev;
        explicit Accounting(proxsdp_model& m) : prev(proxsdp::DevAccount::sink) { proxsdp::DevAccount::sink = &m.bytes; }
        ~Accounting() { proxsdp::DevAccount::sink = prev; }
    };

    // o: validated options; the caller has refused what a handle does not serve
    proxsdp_model(const proxsdp_problem& prob, const proxsdp_options& o) : opt0(o), index_base(prob.index_base) {
        using namespace proxsdp;
        const double t0 = now_s();
        Accounting acct(*this);
        S.reset(new Solver(prob, o, scratch, nullptr, 0, true));      // prepare(): every check of proxsdp_hip_solve, on the host
        Solver& s = *S;
        size_t rlen = 0;
        for (const BlockInfo& B : s.P.blocks) rlen += (size_t)B.n;
        if (prob.eig_resid) { resid.assign(prob.eig_resid, prob.eig_resid + rlen); s.user_resid = resid.data(); }
        psd_ptr.assign(1, 0);
        for (const BlockInfo& B : s.P.blocks) psd_ptr.push_back(psd_ptr.back() + B.N);
        shape.n = s.P.n; shape.p = s.P.p; shape.m = s.P.m;
        shape.n_psd = (int64_t)s.P.blocks.size(); shape.psd_ptr = psd_ptr.data();
        s.req.device_exit = true;
        s.setup();
        s.exit_device_setup();
        const Prep& P = s.P;
        const size_t n1 = (size_t)std::max<int64_t>(P.n, 1);
        static_assert(sizeof(long long) == sizeof(int64_t), "the variable order is uploaded as it is");
        ord_d.alloc(n1); ord_d.upload(reinterpret_cast<const long long*>(P.ord.data()), P.n, s.stream);
        flag_d.alloc(8);
        upload_support_map();
        PX_HIP(hipStreamSynchronize(s.stream));
        s.release_host_threads();
        setup_time = now_s() - t0;
    }

    // position in the support list of every variable (-1: outside), for k_model_c's store into the compact cS
    void upload_support_map() {
        using namespace proxsdp;
        Solver& s = *S;
        if (!s.use_support) return;
        std::vector<int> sinv((size_t)std::max<int64_t>(s.P.n, 1), -1);
        for (int q = 0; q < s.ns; ++q) sinv[s.supp_h[q]] = q;
        sinv_d.alloc(sinv.size());
        sinv_d.upload(sinv.data(), sinv.size(), s.stream);
        PX_HIP(hipStreamSynchronize(s.stream));
    }

    // every stream of the solver idle (after a solve that ended in an exception: launches may still be in flight)
    void drain() {
        proxsdp::Solver& s = *S;
        if (s.stream.main) (void)hipStreamSynchronize(s.stream.main);
        for (proxsdp::EigWork& W : s.eig) {
            if (W.stream) (void)hipStreamSynchronize(W.stream);
            if (W.side) (void)hipStreamSynchronize(W.side);
        }
        (void)hipGetLastError();
    }

    // run: the fields of the options a solve may change, already validated against opt0 (null: opt0's); request: checked
    // by the entry, device_exit set
    void solve(double t_entry, const proxsdp_options* run, proxsdp_result* res, const proxsdp::SolveRequest& request) {
        using namespace proxsdp;
        Solver& s = *S;
        PX_HIP(hipSetDevice(opt0.device_id));
        Accounting acct(*this);
        const proxsdp_options& r = run ? *run : opt0;
        s.opt.time_limit = r.time_limit; s.opt.max_iter = r.max_iter; s.opt.log_verbose = r.log_verbose;
        s.opt.log_freq = r.log_freq; s.opt.warn_on_limit = r.warn_on_limit; s.opt.trace_capacity = r.trace_capacity;
        if (s.opt.trace_capacity > 0 && !res->trace) s.opt.trace_capacity = 0;
        scratch = *res;
        s.time0 = t_entry; s.t_init0 = t_entry;
        struct Leave {                                      // no thread of the handle outlives the call
            proxsdp_model& m; bool ok = false;
            ~Leave() { if (!ok) m.drain(); m.S->release_host_threads(); }
        } leave{*this};
        s.reset_for_solve();
        s.req = request;
        s.start_block_workers();
        s.solve();
        PX_HIP(hipStreamSynchronize(s.stream));
        leave.ok = true;
        *res = scratch;
        ++solves;
    }

    // upd: validated on the host (struct_size, some pointer given, host values finite, what the model does not serve)
    void update(const proxsdp_model_data& u) {
        using namespace proxsdp;
        Solver& s = *S;
        Prep& P = s.P;
        RowState& rs = s.rs;
        PX_HIP(hipSetDevice(opt0.device_id));
        Accounting acct(*this);
        hipStream_t st = s.stream;
        const bool on_dev = u.on_device != 0;
        const int64_t nnzA = P.nnzA, nnzG = P.nnz - P.nnzA;
        const double* src[5] = {u.c, u.b, u.h, u.A_nzval, u.G_nzval};
        const int64_t len[5] = {P.n, P.p, P.m, nnzA, nnzG};
        const char* name[5] = {"c", "b", "h", "A_nzval", "G_nzval"};
        if (on_dev) require_finite_device(st, flag_d, 5, src, len, name, "proxsdp_model_data");
        s.restore_cert_data();                              // (a certificate search of the last solve zeroed c or [b; h])
        // a host array goes through the staging buffer; the stream orders its reuse
        auto on_device = [&](int q) -> const double* {
            if (on_dev || !src[q] || len[q] == 0) return src[q];
            if (stage.n < (size_t)len[q]) stage.alloc((size_t)std::max<int64_t>(std::max(P.n, P.Q), std::max<int64_t>(P.nnz, 1)));
            stage.upload(src[q], (size_t)len[q], st);
            return stage.p;
        };
        const double cte = std::sqrt(2.0) / 2.0;
        int moved = 0;
        if (u.c && P.n > 0) {
            const double* d = on_device(0);
            PX_HIP(hipMemsetAsync(flag_d.p + 5, 0, sizeof(int), st));
            hipLaunchKernelGGL(dev::k_model_c, dim3(grid_for(P.n)), dim3(dev::TPB), 0, st, d, (const long long*)ord_d.p,
                               (const unsigned char*)s.offdiag_d.p, cte, (const int*)rs.csc_ptr.p,
                               s.use_support ? (const int*)sinv_d.p : (const int*)nullptr, s.c_d.p, s.xd.c.p,
                               s.use_support ? s.cS_d.p : (double*)nullptr, flag_d.p + 5, (long long)P.n);
            PX_HIP(hipGetLastError());
            if (on_dev) P.norm_c = model_norm2(st, d, P.n, npart, nout);
            else P.norm_c = norm2(u.c, P.n);
            PX_HIP(hipMemcpyAsync(&moved, flag_d.p + 5, sizeof(int), hipMemcpyDeviceToHost, st));
            s.c_d.download(P.c.data(), P.n, st);
            s.xd.c.download(P.c_orig.data(), P.n, st);
            PX_HIP(hipStreamSynchronize(st));
            s.c_host = P.c;
        }
        for (int q = 3; q < 5; ++q) {
            if (!src[q] || len[q] == 0) continue;
            const int64_t off = q == 3 ? 0 : nnzA;
            const double* d = on_device(q);
            hipLaunchKernelGGL(dev::k_model_values, dim3(grid_for(len[q])), dim3(dev::TPB), 0, st, d, (long long)len[q],
                               (const int*)rs.csc_pos_d.p + off, (const int*)rs.csr_pos_d.p + off, (const int*)rs.csr_col.p,
                               (const unsigned char*)s.offdiag_d.p, cte, rs.exit.cval.p, rs.exit.rval.p, rs.csc_val.p, rs.csr_val.p);
            PX_HIP(hipGetLastError());
        }
        if ((u.A_nzval && nnzA > 0) || (u.G_nzval && nnzG > 0)) {
            rs.csc_val.download(P.val.data(), P.nnz, st);
            rs.csr_val.download(P.rval.data(), P.nnz, st);
            rs.exit.cval.download(P.val_orig.data(), P.nnz, st);
            PX_HIP(hipStreamSynchronize(st));
            P.frob = on_dev ? model_norm2(st, rs.csc_val.p, P.nnz, npart, nout) : host_frob(P);
        }
        if ((u.b && P.p > 0) || (u.h && P.m > 0)) {
            const double* db = nullptr;
            const double* dh = nullptr;
            if (u.b && P.p > 0) {
                db = on_device(1);
                if (!on_dev) {                              // (the staging buffer takes h next: b's launch goes first)
                    hipLaunchKernelGGL(dev::k_model_bh, dim3(grid_for(P.Q)), dim3(dev::TPB), 0, st, db, (long long)P.p,
                                       (const double*)nullptr, (long long)P.m, rs.bh_d.p, rs.exit.bh.p);
                    db = nullptr;
                }
            }
            if (u.h && P.m > 0) dh = on_device(2);
            if (db || dh)
                hipLaunchKernelGGL(dev::k_model_bh, dim3(grid_for(P.Q)), dim3(dev::TPB), 0, st, db, (long long)P.p, dh,
                                   (long long)P.m, rs.bh_d.p, rs.exit.bh.p);
            PX_HIP(hipGetLastError());
            if (u.b && P.p > 0) P.norm_b = on_dev ? model_norm2(st, u.b, P.p, npart, nout) : norm2(u.b, P.p);
            if (u.h && P.m > 0) P.norm_h = on_dev ? model_norm2(st, u.h, P.m, npart, nout) : norm2(u.h, P.m);
            std::vector<double> bh((size_t)P.Q);
            rs.bh_d.download(bh.data(), P.Q, st);
            PX_HIP(hipStreamSynchronize(st));
            std::copy(bh.begin(), bh.begin() + P.p, P.b.begin());
            std::copy(bh.begin() + P.p, bh.end(), P.h.begin());
            P.b_orig = P.b; P.h_orig = P.h;
            s.b_host = P.b; s.h_host = P.h;
        }
        PX_HIP(hipStreamSynchronize(st));
        if (moved != 0) rebuild_support();
        ++updates;
    }

    // the support set changed: what setup_support() and alloc_candidates() built, again
    void rebuild_support() {
        using namespace proxsdp;
        Solver& s = *S;
        for (EigWork& W : s.eig) { W.fop_ok = false; W.ell_w = 0; W.ov = dev::EllOverflow{}; }
        s.ns = 0; s.rstride = 0; s.n_res_wg = 0; s.tile_base.clear(); s.supp_h.clear();
        s.setup_support();
        s.alloc_candidates();
        upload_support_map();
        ++support_rebuilds;
    }

    // ch: validated on the host as far as no model is needed (check_rows_struct); the model's own refusals are the caller's.
    // Order: plan (host; the last refusals) -> the finite check of device values -> build: a second RowState for the plan's
    // shape and the plan's source maps -> fill: the pattern, the gathers from the live state, the host mirrors, the two norms
    // -> swap: the two states exchanged, the Prep's changed members committed -> the support set, where it moved.
    void change_rows(proxsdp_model_rows& ch) {
        using namespace proxsdp;
        const double t0 = now_s();
        Solver& s = *S;
        Prep& P = s.P;
        RowsPlan pl = plan_rows(P, index_base, ch);
        PX_HIP(hipSetDevice(opt0.device_id));
        Accounting acct(*this);
        AllocCount counting;
        hipStream_t st = s.stream;
        const bool on_dev = ch.on_device != 0;
        const int64_t na = ch.n_add, nnz_add = pl.nnz_add;
        if (on_dev && na > 0) {
            const double* src[2] = {ch.add_val, ch.add_h};
            const int64_t len[2] = {nnz_add, na};
            const char* name[2] = {"add_val", "add_h"};
            require_finite_device(st, flag_d, 2, src, len, name, "proxsdp_model_rows");
        }
        s.restore_cert_data();                              // (a certificate search of the last solve zeroed c or [b; h])
        bool supp_moved = false;                            // only a column that lost or gained an entry can enter or leave the set
        for (int32_t k : pl.touched) supp_moved = supp_moved || in_support(P.colptr, P.c, k) != in_support(pl.R.colptr, P.c, k);
        Prep& R = pl.R;
        const RowState& old = s.rs;
        // ---- build: the next row state and the source maps, before the first write and before an old buffer goes
        const size_t nz = (size_t)std::max<int64_t>(R.nnz, 1), q1 = (size_t)std::max<int64_t>(R.Q, 1);
        RowState next;
        next.build(R.n, R.p, R.m, R.nnz, true);
        next.build_exit(R.p, R.m, R.nnz, s.exit_feas_grid(R.m));
        DevBuf<int> csc_src(nz), csr_src(nz), bh_src(q1), add_k((size_t)std::max<int64_t>(nnz_add, 1));
        const double* d_val = ch.add_val;
        const double* d_h = ch.add_h;
        if (!on_dev && na > 0) {                            // host values: through the staging buffer, the two arrays side by side
            const size_t need = (size_t)(nnz_add + na);
            if (stage.n < need) stage.alloc(std::max(need, (size_t)std::max<int64_t>(std::max(R.n, R.Q), std::max<int64_t>(R.nnz, 1))));
            stage.upload(ch.add_val, (size_t)nnz_add, st);
            PX_HIP(hipMemcpyAsync(stage.p + nnz_add, ch.add_h, (size_t)na * sizeof(double), hipMemcpyHostToDevice, st));
            d_val = stage.p; d_h = stage.p + nnz_add;
        }
        // ---- fill: the pattern and the mat-vec's shape from the plan, the numbers through the source maps
        s.upload_pattern(next, R);
        csc_src.upload(pl.csc_src.data(), R.nnz, st); csr_src.upload(pl.csr_src.data(), R.nnz, st);
        bh_src.upload(pl.bh_src.data(), R.Q, st); add_k.upload(pl.add_k.data(), nnz_add, st);
        const double cte = std::sqrt(2.0) / 2.0;
        if (R.nnz > 0) {
            hipLaunchKernelGGL(dev::k_rows_values, dim3(grid_for(R.nnz)), dim3(dev::TPB), 0, st, (const int*)csc_src.p, (long long)R.nnz,
                               (const double*)old.exit.cval.p, (const double*)old.csc_val.p, d_val, (const int*)add_k.p,
                               (const unsigned char*)s.offdiag_d.p, cte, next.exit.cval.p, next.csc_val.p);
            hipLaunchKernelGGL(dev::k_rows_values, dim3(grid_for(R.nnz)), dim3(dev::TPB), 0, st, (const int*)csr_src.p, (long long)R.nnz,
                               (const double*)old.exit.rval.p, (const double*)old.csr_val.p, d_val, (const int*)add_k.p,
                               (const unsigned char*)s.offdiag_d.p, cte, next.exit.rval.p, next.csr_val.p);
        }
        if (R.Q > 0)
            hipLaunchKernelGGL(dev::k_rows_bh, dim3(grid_for(R.Q)), dim3(dev::TPB), 0, st, (const int*)bh_src.p, (long long)R.Q,
                               (const double*)old.bh_d.p, d_h, next.bh_d.p, next.exit.bh.p);
        PX_HIP(hipGetLastError());
        for (int k = 0; k < 2; ++k) { next.ybuf[k].zero(st); next.Mxbuf[k].zero(st); }
        next.ycand_d.zero(st); next.exit.slack.zero(st);
        // the host mirrors, the way update brings them up to date: from the device arrays
        next.csc_val.download(R.val.data(), R.nnz, st);
        next.csr_val.download(R.rval.data(), R.nnz, st);
        next.exit.cval.download(R.val_orig.data(), R.nnz, st);
        std::vector<double> bhh((size_t)R.Q);
        next.bh_d.download(bhh.data(), R.Q, st);
        PX_HIP(hipStreamSynchronize(st));
        std::copy(bhh.begin() + R.p, bhh.end(), R.h.begin());
        R.h_orig = R.h;
        if (on_dev) {
            R.norm_h = model_norm2(st, next.bh_d.p + R.p, R.m, npart, nout);
            R.frob = model_norm2(st, next.csc_val.p, R.nnz, npart, nout);
        } else {
            rows_host_norms(R);
        }
        // ---- swap (nothing throws until the solver and its Prep describe the new rows, no device allocation until the support rebuild)
        std::swap(s.rs, next);
        P.norm_h = R.norm_h; P.frob = R.frob;
        commit_rows(P, pl);
        s.b_host = P.b; s.h_host = P.h;
        shape.m = P.m;
        ch.support_rebuilt = 0;
        // a changed set matters where the support path runs, or would now (the auto rule reads the set's size)
        if (supp_moved && (s.use_support || s.support_path_wanted(s.support_list().size()))) { rebuild_support(); ch.support_rebuilt = 1; }
        PX_HIP(hipStreamSynchronize(st));
        ch.m_new = P.m; ch.nnz_new = P.nnz;
        if (ch.kept) std::copy(pl.kept.begin(), pl.kept.end(), ch.kept);
        ch.bytes_allocated = counting.bytes;
        ch.seconds = now_s() - t0;
    }

    // ---- the tools.  The entry has refused what the host can decide; a method makes the handle's device current, takes the
    // stream and the cone, and calls the tool's driver.  No Accounting: a tool's scratch is the call's.

    // the PSD cone a struct names, or the refusal under the struct's name
    const proxsdp::BlockInfo& cone(int64_t k, const char* who) const {
        const std::vector<proxsdp::BlockInfo>& blocks = S->P.blocks;
        if (k < 0 || k >= (int64_t)blocks.size()) throw std::invalid_argument(std::string(who) + ".cone is outside the model's PSD cones");
        return blocks[(size_t)k];
    }
    hipStream_t enter() {
        PX_HIP(hipSetDevice(opt0.device_id));
        return S->stream;
    }

    // the cone's variable list (0-based caller numbers) on the host and on the device: what the cut tools read
    void triangles(proxsdp_triangle_cuts& tc) {
        const proxsdp::BlockInfo& B = cone(tc.cone, "proxsdp_triangle_cuts");
        proxsdp::device_triangle_cuts(enter(), S->P.ord.data() + B.off, ord_d.p + B.off, B.n, index_base, tc.cone, tc);
    }
    void cliques(proxsdp_clique_cuts& q) {
        const proxsdp::BlockInfo& B = cone(q.cone, "proxsdp_clique_cuts");
        proxsdp::device_clique_cuts(enter(), S->P.ord.data() + B.off, ord_d.p + B.off, B.n, index_base, q.cone, q);
    }
    void inactive_rows(proxsdp_inactive_rows& q) { proxsdp::inactive_rows(enter(), S->P.m, q); }

    // The objective is the exit path's unscaled c, where the cone's entries are contiguous
    void round(proxsdp_rounding& q) {
        const proxsdp::BlockInfo& B = cone(q.cone, "proxsdp_rounding");
        hipStream_t st = enter();
        S->restore_cert_data();                             // (a certificate search of the last solve zeroed c or [b; h])
        proxsdp::device_round(st, S->xd.c.p + B.off, B.n, q.cone, q);
    }

    // the model is one the call serves (the entry's refusals)
    void bound(proxsdp_dual_bound& q) {
        proxsdp::Solver& s = *S;
        hipStream_t st = enter();
        s.restore_cert_data();                              // (a certificate search of the last solve zeroed c or [b; h])
        const proxsdp::BoundModel md{s.P, s.rs.csc_ptr.p, s.rs.csc_row.p, s.rs.exit.cval.p, s.rs.exit.bh.p, s.xd.c.p, s.offdiag_d.p};
        proxsdp::device_dual_bound(st, md, q);
    }

    void info(proxsdp_model_info& out) const {
        const proxsdp::Solver& s = *S;
        out.n = s.P.n; out.p = s.P.p; out.m = s.P.m; out.n_psd = (int64_t)s.P.blocks.size(); out.nnz = s.P.nnz;
        out.device_id = opt0.device_id; out.use_support = s.use_support ? 1 : 0;
        out.solves = solves; out.updates = updates; out.support_rebuilds = support_rebuilds;
        out.device_bytes = bytes.load();
        out.setup_time = setup_time;
    }

    // sizes always; an array when its pointer is given
    void dump(proxsdp_model_dump& out) {
        using namespace proxsdp;
        Solver& s = *S;
        const Prep& P = s.P;
        const RowState& rs = s.rs;
        PX_HIP(hipSetDevice(opt0.device_id));
        s.restore_cert_data();
        hipStream_t st = s.stream;
        out.n = P.n; out.Q = P.Q; out.nnz = P.nnz; out.ns = s.use_support ? s.ns : 0;
        out.norms[0] = P.norm_b; out.norms[1] = P.norm_h; out.norms[2] = P.norm_c; out.norms[3] = P.frob;
        if (out.csc_val) rs.csc_val.download(out.csc_val, P.nnz, st);
        if (out.csr_val) rs.csr_val.download(out.csr_val, P.nnz, st);
        if (out.csc_val_orig) rs.exit.cval.download(out.csc_val_orig, P.nnz, st);
        if (out.csr_val_orig) rs.exit.rval.download(out.csr_val_orig, P.nnz, st);
        if (out.c) s.c_d.download(out.c, P.n, st);
        if (out.c_orig) s.xd.c.download(out.c_orig, P.n, st);
        if (out.bh) rs.bh_d.download(out.bh, P.Q, st);
        if (out.support && out.ns > 0) PX_HIP(hipMemcpyAsync(out.support, s.supp_d.p, (size_t)out.ns * sizeof(int), hipMemcpyDeviceToHost, st));
        if (out.cS && out.ns > 0) s.cS_d.download(out.cS, out.ns, st);
        PX_HIP(hipStreamSynchronize(st));
    }
};
