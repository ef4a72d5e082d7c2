/*
 * proxsdp_hip.h -- C ABI of libproxsdp_hip.so, the MI355X (gfx950) implementation
 * of ProxSDP's PDHG hot path.
 *
 * Drop-in boundary.  The reference has no FFI: its solver is entered through ONE
 * call, `sol = chambolle_pock(aff, con, options)` at
 * /root/reference/src/MOI_wrapper.jl:310 (inside `_optimize!`, :220-342).
 * `proxsdp_hip_solve` replaces exactly that call: its three arguments carry
 *     AffineSets + ConicSets   /root/reference/src/structs.jl:32-58
 *     Options                  /root/reference/src/options.jl:1-132
 *     Result                   /root/reference/src/structs.jl:60-81
 * A Julia binding calls it with `ccall` (see INTEGRATION.md and julia/); the
 * Python ctypes binding in proxsdp.jl_amd/binding.py is what the tests use.
 *
 * Conventions
 *   - plain C, no C++/torch types; pointers are HOST pointers unless a field says
 *     otherwise (the two exceptions: `M_dense` with M_dense_on_device = 1 and the
 *     buffer handed to `reduce_vec_fn` with reduce_vec_on_device = 1 are DEVICE
 *     pointers on options.device_id), borrowed for the duration of the call, never
 *     freed or written by the library (the reference mutates `aff` in place --
 *     scaling.jl:24, pdhg.jl:647-663 -- the library works on private copies).
 *   - index_base = 1 is the Julia calling convention (1-based Int64 colptr / rowval /
 *     cone variable lists, structs.jl:32-53); exercised without Julia by
 *     tests/test_julia_convention.py (ctypes with 1-based arrays + a plain-C caller).
 *   - return value: 0 = the solve ran to a solver status (whatever it is);
 *     < 0 = the call failed (PROXSDP_E_*), text in proxsdp_hip_last_error().
 *     Nothing unwinds across the ABI.  There is NO CPU fallback: without a
 *     usable HIP device every compute entry point returns PROXSDP_E_HIP.
 *   - Float64 arithmetic throughout (the reference is Float64 only).
 */
#ifndef PROXSDP_HIP_H
#define PROXSDP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7 (round 3): proxsdp_options gained sign_start_row and general_batch (taken from reserved_i), proxsdp_stats gained
 * sign_short_pass / sign_short_fail (taken from reserved): same struct sizes and offsets as version 6
 * 8 (round 4): proxsdp_options gained full_eig_lanczos_certify (from reserved_i) and full_eig_lanczos_tol (from
 * reserved_d) and host_merge_threads (from reserved_i), proxsdp_stats full_eigs_lanczos_certified / _cert_failed /
 * cert_matvecs (the last reserved slots):
 * same struct sizes and offsets; debug_fail_iteration now needs PROXSDP_HIP_FAULT_INJECTION=1
 * 9 (round 5): proxsdp_options grew at its END (equilibration_reference_aliasing, block_batch_groups,
 * new reserved slots -- offsets of every earlier member unchanged, struct_size larger), proxsdp_stats grew at its end
 * (proxsdp_result with it: it is the LAST member); a Krylov dimension beyond 255 is served by the dense eigensolver
 * instead of PROXSDP_E_INVALID; new proxsdp_state and
 * proxsdp_hip_solve_ex (capture / resume of the solver state at an iteration boundary); PROXSDP_E_COMM_ABORTED;
 * later: proxsdp_options gained lanczos_wide_krylov (from reserved_i2[0]), proxsdp_stats wide_krylov_projections
 * (from reserved_s[0]): same struct sizes and offsets, version unchanged;
 * later: proxsdp_options gained device_eig_merge (the LAST slot of reserved_i2), proxsdp_stats.reserved_s[1..2] count the device
 * merges and their fallbacks (PROXSDP_STATS_DEVICE_EIG_MERGES / _FALLBACKS), new test entry proxsdp_device_symeig_split: same
 * sizes and offsets, version unchanged;
 * later: equilibration and approx_norm = 0 served with a dense A (proxsdp_hip_dense_scaling, proxsdp_host_equilibrate_rowsums),
 * proxsdp_stats dense_setup_passes / dense_sigma_steps (the last two reserved_s slots): same sizes and offsets, version unchanged;
 * later: a block-sharded solve accepts SOC cones, 1x1 PSD cones and variables outside every cone (such a shard runs the general
 * vector path); proxsdp_stats.reserved_s[0] counts its iterations (PROXSDP_STATS_SHARDED_GENERAL_ITERATIONS); proxsdp_trial_batch
 * support = 2: same sizes and offsets, version unchanged;
 * later: proxsdp_hip_solve_sharded (a whole model, split by the library, one shard per host thread and device of ONE process),
 * with its test entries proxsdp_host_split_shard, proxsdp_host_group_reduce, proxsdp_hip_coupling_sum: functions only, no
 * struct changed -- as for proxsdp_hip_dense_scaling before, the version stays;
 * later: proxsdp_stats.reserved_s[3] counts the Lanczos steps on the owner form of the operator-form mat-vec
 * (PROXSDP_STATS_FOP_OWNER_STEPS; switch: environment PROXSDP_HIP_FOP_OWNER): same sizes and offsets, version unchanged;
 * later: proxsdp_hip_solve_factored (the low-rank factors of the PSD solution beside the result) with the new struct
 * proxsdp_psd_factors and the test entries proxsdp_hip_factor_residual / _kernel: functions and one new struct, no existing
 * struct changed: the version stays;
 * later: proxsdp_hip_solve_from (warm start from a previous solution's primal / duals / factors) with the new struct
 * proxsdp_start and the test entry proxsdp_hip_start_point: functions and one new struct, the version stays;
 * later: the test entries proxsdp_hip_reconstruct_fused, proxsdp_hip_rotate and proxsdp_hip_tail_copy with their own structs:
 * functions and new structs, no existing struct changed: the version stays;
 * later: the model handle (proxsdp_hip_model_create / _update / _solve / _info / _destroy: a model that stays set up on the
 * device between solves) with the new structs proxsdp_model_data, proxsdp_model_info and proxsdp_model_dump and the test
 * entries proxsdp_hip_model_dump, proxsdp_hip_model_norm2 and proxsdp_host_model_prepare: functions and new structs, no
 * existing struct changed: the version stays;
 * later: proxsdp_hip_model_rows (inequality rows of a model handle added and dropped in place) with the new struct
 * proxsdp_model_rows and the test entry proxsdp_host_model_rows_plan: functions and one new struct, no existing struct
 * changed: the version stays;
 * later: proxsdp_hip_model_triangles (the most violated triangle inequalities of a PSD cone of a model handle, separated on
 * the device) with its host restatement proxsdp_host_triangle_cuts, and proxsdp_hip_model_inactive_rows (the inequality rows
 * that went slack), with the new structs proxsdp_triangle_cuts and proxsdp_inactive_rows: functions and two new structs, no
 * existing struct changed: the version stays;
 * later: proxsdp_hip_model_round (randomised hyperplane rounding of a PSD cone's factors to +-1 vectors and a one-flip local
 * search against the handle's current objective, on the device) with its host restatement proxsdp_host_round and the
 * direction generator proxsdp_host_round_directions, with the new struct proxsdp_rounding: functions and one new struct, no
 * existing struct changed: the version stays;
 * later: the test entry proxsdp_hip_lanczos_cycles (every cycle of a thick-restart Lanczos run, as the driver leaves it) with
 * the new struct proxsdp_lanczos_cycles: one function and one new struct, no existing struct changed: the version stays;
 * later: proxsdp_hip_model_cliques (pentagonal and heptagonal odd-clique inequalities of a PSD cone of a model handle, grown
 * from triangles or pentagons on the device) with its host restatement proxsdp_host_clique_cuts and the new struct
 * proxsdp_clique_cuts: two functions and one new struct, no existing struct changed: the version stays
 * later: proxsdp_hip_model_bound (a certified lower bound of a model handle's optimum from any dual point: the proof is a
 * completed fp64 Cholesky factorisation on the device with its backward-error bound) with its host restatement
 * proxsdp_host_dual_bound, the test entries proxsdp_hip_cholesky / proxsdp_host_cholesky and the new struct
 * proxsdp_dual_bound: four functions and one new struct, no existing struct changed: the version stays;
 * later: the test entry proxsdp_hip_project_cones (one PSD projection of a vector of mixed cones through the solver's own
 * set-up and launch code) with the new struct proxsdp_project_cones: one function and one new struct, no existing struct
 * changed: the version stays;
 * later: the test entry proxsdp_hip_operator_cycles (every cycle of a Lanczos run on the operator form: the block given as a
 * support list, its values and the previous projection's factors) with the new struct proxsdp_operator_cycles, and the host
 * entry proxsdp_host_block1_lds_doubles (the LDS plan of the one-workgroup cycle kernel): two functions and one new struct, no
 * existing struct changed: the version stays;
 * later: the test entry proxsdp_hip_positive_part (one positive-part run of the Lanczos engine through the same observer, and
 * its per-call certificate on the run's or on given locked pairs) with the new struct proxsdp_positive_part: one function and
 * one new struct, no existing struct changed: the version stays */
#define PROXSDP_HIP_ABI_VERSION 10

/* error codes (negative return values) */
#define PROXSDP_E_INVALID  (-1)   /* invalid argument / inconsistent problem data */
#define PROXSDP_E_HIP      (-2)   /* HIP runtime / rocSOLVER failure, no device   */
#define PROXSDP_E_NOMEM    (-3)   /* host or device allocation failed             */
#define PROXSDP_E_UNSUPP   (-4)   /* option combination not implemented           */
#define PROXSDP_E_INTERNAL (-5)
#define PROXSDP_E_COMM_ABORTED (-6) /* block-sharded solve on the native RCCL path: the solve failed AND the library called
                                     * ncclCommAbort on proxsdp_problem.nccl_comm -- the communicator is already released:
                                     * it must NOT be destroyed or used again by the caller */

/* solver status: Result.status, /root/reference/src/MOI_wrapper.jl:381-399 */
#define PROXSDP_STATUS_NOT_CALLED       0
#define PROXSDP_STATUS_OPTIMAL          1
#define PROXSDP_STATUS_TIME_LIMIT       2
#define PROXSDP_STATUS_ITERATION_LIMIT  3
#define PROXSDP_STATUS_INFEAS_OR_UNBND  4
#define PROXSDP_STATUS_DUAL_INFEASIBLE  5
#define PROXSDP_STATUS_INFEASIBLE       6

/* SparseMatrixCSC{Float64,Int64} (structs.jl:36-37) */
typedef struct proxsdp_csc {
    int64_t nrows;
    int64_t ncols;
    const int64_t* colptr;   /* ncols+1 entries, base = problem.index_base */
    const int64_t* rowval;   /* nnz entries,     base = problem.index_base */
    const double*  nzval;    /* nnz entries */
} proxsdp_csc;

/* AffineSets + ConicSets as assembled at MOI_wrapper.jl:229-292:
 *   minimise c'x   s.t.  A x = b,  G x <= h,  x restricted to the cones.
 * PSD cones are MOI PositiveSemidefiniteConeTriangle variable lists (upper
 * triangle, column by column); SOC cones are (t, x...) variable lists. */
typedef struct proxsdp_problem {
    int64_t n;                 /* number of scalar variables            (aff.n) */
    int64_t p;                 /* equality rows                         (aff.p) */
    int64_t m;                 /* inequality rows                       (aff.m) */
    proxsdp_csc A;             /* p x n */
    proxsdp_csc G;             /* m x n */
    const double* b;           /* p */
    const double* h;           /* m */
    const double* c;           /* n, already sign-flipped for MAX sense (:252-255) */
    int64_t n_psd;
    const int64_t* psd_ptr;    /* n_psd+1 offsets into psd_idx (0-based offsets)   */
    const int64_t* psd_idx;    /* SDPSet.vec_i of every cone, concatenated         */
    int64_t n_soc;
    const int64_t* soc_ptr;    /* n_soc+1 */
    const int64_t* soc_idx;    /* SOCSet.idx concatenated */
    int32_t index_base;        /* 0 or 1: base of colptr/rowval/psd_idx/soc_idx    */
    int32_t reserved0;
    /* optional (may be NULL): Lanczos start vectors, one per PSD cone, sides
     * concatenated.  The reference uses normalize!(randn(MersenneTwister(seed), n))
     * (eigsolver.jl:392-411), which only Julia can generate; when NULL the library
     * uses its own counter-based generator (csrc/host_util.hpp, mirrored in
     * oracle/eig.py:start_vector). */
    const double* eig_resid;
    /* optional block-sharded solve (multi-GPU, one process per GPU).
     * When reduce_fn != NULL this problem is ONE SHARD of a model whose cones are distributed over
     * the shards (the cones it owns -- PSD blocks of any side, 1x1 included, SOC cones -- the
     * variables outside every cone it owns, and the constraint rows that touch only them; rows that
     * touch several shards are coupling rows, below).  A shard may hold no PSD block at all.  A shard
     * with at least one PSD block, no SOC and no 1x1 block runs the support-aware vector path, any
     * other shard the general one; shards of one solve may differ.  Not served in a sharded solve:
     * approx_norm = 0, equilibration, M_dense, the state seam.  The library calls
     *     reduce_fn(reduce_ctx, sums, nsum, maxs, nmax)
     * with host arrays; the callee must replace sums[] by the element-wise SUM and maxs[] by
     * the element-wise MAX over all shards (e.g. two RCCL all-reduces) and return 0.  It is
     * called once at start-up and once per PDHG iteration (plus rare extra calls: another
     * linesearch batch, check_dual_feas, the global SOC stop test -- which every shard enters,
     * SOC-free ones included -- and the exit path), by every
     * shard in the same order.  Only scalars cross shards: the reference's serial loop over
     * blocks (prox_operators.jl:40) becomes one block set per GPU. */
    void* reduce_ctx;
    int (*reduce_fn)(void* ctx, double* sums, int32_t nsum, double* maxs, int32_t nmax);
    /* optional dense equality block, for models whose A_k are all dense (test/base_randsdp.jl:
     * 4-23: n = 2000, m = 4000 gives 8.0e9 entries = 64 GB, beyond a sparse index type and
     * pointless to index).  When M_dense != NULL it is A as a ROW-MAJOR p x n array of doubles,
     * columns in the caller's variable order; the CSC `A` is then ignored (its pointers may be
     * NULL) while G stays sparse (e.g. the variable bounds of test/moi_randsdp.jl:33-45).
     * M_dense_on_device = 1: a device pointer on options.device_id (e.g. generated there);
     * 0: host memory, uploaded once.  Borrowed and never modified either way (the reference
     * scales aff.A in place, scaling.jl:24; here the column scaling is applied to the
     * vectors).  Restrictions: the variables must already be in solver order (cone variables
     * first, in cone order: psd_idx/soc_idx concatenated = 0,1,2,...), and reduce_fn must be
     * NULL. */
    const double* M_dense;
    int32_t M_dense_on_device;
    int32_t reserved1;
    /* optional, block-sharded solves only: COUPLING ROWS -- rows of [A;G] with entries in the variables
     * of more than one shard.  Every shard lists the same n_coupling rows (its own
     * 0-BASED row numbers, whatever index_base: 0..p-1 equalities, p..p+m-1 inequalities; a shard without entries in such a row still
     * carries it, empty, with the same right-hand side) in the SAME order.  Per iteration the library
     * hands the shard's partial (M x) of these rows to
     *     reduce_vec_fn(reduce_ctx, buf, n_coupling, on_device)
     * which must replace buf[] by the element-wise SUM over all shards (one RCCL all-reduce on a
     * device buffer when reduce_vec_on_device = 1, host memory otherwise) and return 0 after the
     * result is in place.  coupling_owned[k] = 1 on exactly ONE shard per row: that shard counts
     * the row in the scalar sums (b'y, h'y, |y+ - y|^2, ...), the others skip it -- on both vector
     * paths.  Which variables a shard owns is the caller's choice (whole cones; free variables
     * anywhere): a poor assignment only makes more rows coupling rows, up to all of them. */
    int64_t n_coupling;
    const int64_t* coupling_rows;
    const int32_t* coupling_owned;
    int (*reduce_vec_fn)(void* ctx, double* buf, int64_t len, int32_t on_device);
    int32_t reduce_vec_on_device;
    int32_t reserved2;
    /* optional, block-sharded solves only: an RCCL communicator (ncclComm_t, one rank per shard, created by the
     * caller -- e.g. ncclCommInitRank in the process that owns the GPU).  When non-NULL the library issues BOTH
     * collectives itself on its own stream -- ncclAllReduce(sum) / ncclAllReduce(max) of the packed scalar record
     * and ncclAllReduce(sum) of the coupling buffer -- with no host callback and no host copy of the vectors;
     * reduce_fn / reduce_vec_fn may then be NULL (they are ignored).  librccl.so is loaded at run time
     * (dlopen): the library does not link it, and a process that never passes a communicator never loads it.
     * Every host wait behind one of these collectives is bounded (PROXSDP_HIP_COLLECTIVE_TIMEOUT_S seconds, default
     * 300): a rank whose peer left the solve aborts its communicator (ncclCommAbort) and returns
     * PROXSDP_E_COMM_ABORTED instead of waiting for ever; a rank that fails for its own reasons AFTER its first collective
     * was enqueued aborts its communicator on the way out and returns PROXSDP_E_COMM_ABORTED as well (a failure before any
     * collective -- argument errors -- leaves the communicator untouched and returns the ordinary error code).
     * ncclCommAbort RELEASES the communicator: after PROXSDP_E_COMM_ABORTED the handle is dead -- do not pass it to
     * proxsdp_hip_rccl_comm_destroy / ncclCommDestroy, do not reuse it. */
    void* nccl_comm;
    int64_t reserved3;
} proxsdp_problem;

/* Options (options.jl:1-132): same names, same defaults (proxsdp_hip_default_options).
 * Booleans are int32 0/1.  Fields that have no use in the reference's src/ are kept
 * for name parity and ignored (convergence_check, min_beta, max_beta, reduce_rank,
 * warm_start_eig, disable_julia_logger, timer_*). */
typedef struct proxsdp_options {
    int64_t struct_size;       /* = sizeof(proxsdp_options), set by default_options */
    /* printing */
    int32_t log_verbose;  int32_t log_freq;
    int32_t timer_verbose; int32_t timer_file; int32_t disable_julia_logger;
    int32_t warn_on_limit; int32_t extended_log; int32_t extended_log2; int32_t log_repeat_header;
    int32_t pad0;
    double  time_limit;
    /* tolerances */
    double tol_gap, tol_feasibility, tol_feasibility_dual, tol_primal, tol_dual, tol_psd, tol_soc;
    int32_t check_dual_feas; int32_t check_dual_feas_freq;
    double  max_obj; int32_t min_iter_max_obj; int32_t pad1;
    /* infeasibility */
    int32_t min_iter_time_infeas; int32_t pad2;
    double infeas_gap_tol, infeas_limit_gap_tol, infeas_stable_gap_tol,
           infeas_feasibility_tol, infeas_stable_feasibility_tol;
    int32_t certificate_search; int32_t pad3;
    double certificate_obj_tol, certificate_fail_tol;
    double min_beta, max_beta, initial_beta;
    /* adaptive steps */
    double initial_adapt_level, adapt_decay; int32_t adapt_window; int32_t pad4;
    /* PDHG */
    int32_t convergence_window; int32_t convergence_check;
    int64_t max_iter; int64_t min_iter; int64_t divergence_min_update;
    int64_t max_iter_lp; int64_t max_iter_conic; int64_t max_iter_local;
    int32_t advanced_initialization; int32_t line_search_flag;
    int32_t max_linsearch_steps; int32_t pad5;
    double delta, initial_theta, linsearch_decay;
    /* spectral decomposition */
    int32_t full_eig_decomp; int32_t max_target_rank_krylov_eigs;
    int32_t min_size_krylov_eigs; int32_t warm_start_eig;
    int32_t rank_increment; int32_t rank_increment_factor;
    int32_t eigsolver; int32_t eigsolver_min_lanczos; int64_t eigsolver_resid_seed;
    double  arpack_tol; int32_t arpack_resid_init; int32_t arpack_reset_resid; int64_t arpack_max_iter;
    int32_t krylovkit_reset_resid; int32_t krylovkit_resid_init;
    double  krylovkit_tol; int32_t krylovkit_max_iter; int32_t krylovkit_eager; int32_t krylovkit_verbose;
    int32_t reduce_rank; int32_t rank_slack; int32_t pad6;
    int64_t full_eig_freq; int64_t full_eig_len;
    /* equilibration (equilibration.jl, pdhg.jl:64-92): off by default; `equilibration` alone
     * survives only if min(M)/max(M) > equilibration_limit, `equilibration_force` always.
     * approx_norm = 0: step size from sigma_max(M) instead of ||M||_F (pdhg.jl:108-119).
     * With a dense A (M_dense) both are set up on the device: one extra pass over the matrix for the row sums and the
     * extrema, the scaling carried in the vectors of the dense products (the borrowed matrix is never modified), sigma_max
     * by Lanczos through those products.  Neither is available in a block-sharded solve. */
    int32_t equilibration; int32_t equilibration_iters;
    double  equilibration_lb, equilibration_ub, equilibration_limit;
    int32_t equilibration_force; int32_t approx_norm;
    /* ---- library-only knobs (no reference counterpart) ---- */
    int32_t device_id;         /* HIP device ordinal, default 0                      */
    int32_t trace_capacity;    /* rows available in result.trace (0 = no trace)      */
    int32_t profile_symv_every;/* >0: bracket every k-th symv launch with HIP events  */
    int32_t support_path;      /* -1 auto (default), 0 dense vector passes, 1 force the
                                * support-aware passes when legal */
    int32_t lanczos_operator;  /* mat-vec inside the Lanczos projection: 0 = packed triangle of the
                                * iterate (what dsymv('U') reads, 8 N bytes), 1 = operator form
                                * x_prev(low rank) + sparse update when available (support path;
                                * DESIGN.md section 4), -1 auto = 1 (default) */
    int32_t initial_target_rank; /* reference: 2, hard-coded (pdhg.jl:19-20); a benchmark may start at the
                                  * rank a config names ("rank ~ sqrt(n)"); capped at the block side */
    int32_t full_eig_lanczos;    /* full_eig! (prox_operators.jl:111-126) needs every POSITIVE eigenpair, not the
                                  * whole spectrum: -1 auto / 1 = when the previous projection of the block had few
                                  * positive eigenvalues, compute them with the Lanczos engine (all pairs down to the
                                  * first eigenvalue <= 0, converged to krylovkit_tol) and fall back to the dense
                                  * eigensolver otherwise; 0 = always the dense eigensolver.  Same projection. */
    int32_t lanczos_cycle_kernel;/* 2 (round 6) = ONE WORKGROUP per Lanczos cycle for blocks of side <= 512 (csrc/
                                  * lanczos_block1.hip.hpp: basis in registers, operator and records in LDS, the restart
                                  * rotation in the prologue; the step kernels' arithmetic term by term: BIT-IDENTICAL
                                  * results); applies to the operator form with <= 16 factor columns and to a packed
                                  * triangle that fits in LDS (side <= ~140), Krylov dimension <= 31 -- anything else runs
                                  * the step kernels.  -1 auto = 2 for sides <= 256 (where it is 2.2-2.6x faster per step),
                                  * step kernels beyond; 0 = step kernels always.  1 selected a persistent multi-
                                  * workgroup cycle kernel that has been removed: it now means 0. */
    int32_t lanczos_warm_start;  /* 0 (default): every KrylovKit projection starts from the fixed start vector, as the
                                  * reference does (krylovkit_reset_resid = false).  1: start from the normalised sum of
                                  * the previous projection's Ritz vectors (+ 1e-3 x the fixed vector).  Changes the
                                  * Krylov space, not what is converged (krylovkit_tol).  The Lanczos-served full_eig!
                                  * (full_eig_lanczos: the library's own engine, not KrylovKit's call) warm-starts at 0 and
                                  * 1; -1 = fixed start vector there too. */
    int32_t reconstruct_mfma;    /* rank-r reconstruction V Lam+ V': -1 auto, 0 scalar-FMA kernel, 1 fp64 MFMA
                                  * (v_mfma_f64_16x16x4_f64) kernel */
    int32_t small_block_batch;   /* project the small PSD blocks (never on the Krylov path: side <= min_size_krylov_eigs) in
                                  * ONE launch instead of one dense eigensolver call each: -1 auto = blocks of side 2 by
                                  * the batched Jacobi kernel and blocks of side 3..64 by the one-workgroup, LDS-resident
                                  * sign-function projection (csrc/small_sign.hip.hpp; needs full_eig_sign != 0 and every
                                  * requested tolerance >= 1e-8 -- otherwise auto is ">= 2 blocks of side 2..32, Jacobi");
                                  * 1 = Jacobi for every block of side 2..64; 2 = the sign kernel for every block of
                                  * side 2..64; 0 off */
    int32_t full_eig_sign;       /* full_eig! of a dense block without an eigendecomposition: X+ = (X + X sign(X)) / 2
                                  * with sign(X) from an odd-polynomial iteration of fp64 MFMA products (34 .. 64 products of
                                  * n x n symmetric matrices, see sign_start_row; every |eigenvalue| >= 1e-10 ||X|| is resolved to 1e-15,
                                  * smaller ones contribute an error <= their own size): -1 auto (33 <= n <= 16384 with HBM for the work matrices, and
                                  * every requested tolerance >= 1e-8: below that the 1e-10 floor of this path could
                                  * stall a solve, and the dense eigensolver is used), 1 always, 0 = rocSOLVER dsyevd +
                                  * reconstruction */
    int32_t psd_sign_engine;     /* 1: on the Krylov branch, let the sign-function projection stand in for the Lanczos
                                  * engine when it is measured to be the cheaper way to the SAME matrix (fewer than
                                  * target_rank positive eigenvalues => the truncated projection is the exact one and
                                  * min_eig <= 0; verified after every such projection, redone by Lanczos otherwise;
                                  * on first use and every 64th projection BOTH engines run on the same input and a
                                  * disagreement -- repeated eigenvalues, of which single-vector Lanczos returns one
                                  * copy -- leaves the block to the Lanczos engine for the rest of the solve).
                                  * -1 auto = 0 = off: the reference's engine choice, mat-vec counts as KrylovKit's */
    int32_t full_eig_lanczos_verify; /* full_eig! served by the Lanczos engine (full_eig_lanczos) is the library's own
                                  * algorithm; single-vector Lanczos returns ONE eigenvector per distinct eigenvalue, so a
                                  * repeated positive eigenvalue would silently lose copies.  k > 0: the first such call of a
                                  * block and every k-th after it are ALSO computed by the reference's engine (sign-function /
                                  * dense eigensolver) on the same input and compared (max |difference| <= 1e-8 max |X+|); a
                                  * mismatch hands the block back to the dense engine for the rest of the solve
                                  * (stats.full_eigs_lanczos_checks / _mismatches).  -1 auto = 256, 0 = never */
    double  full_eig_lanczos_posres; /* acceptance of that engine: the first strictly negative Ritz pair must be resolved to
                                  * posres x spectral scale, i.e. a positive eigenvalue the run could have missed is smaller
                                  * than that.  Default 1e-6 -- two orders inside the solver's tolerances (rounds 2-3: 1e-7;
                                  * measured in round 4 on the n = 4000 default solve, with the per-call certificate behind it:
                                  * 1e-7 / 1e-6 / 1e-5 give the same 8651 iterations and objectives equal to 1.4e-14 in
                                  * 12.6 / 11.4 / 9.1 s) */
    int32_t full_eig_lanczos_kdim10; /* its Krylov dimension = max(2 g + 1, g x kdim10 / 10 + 8), default 30 */
    int32_t sign_small_tile_max; /* sign-function projection: 32 x 32 product tiles up to this padded side, 64 x 64
                                  * above (default 3072, measured cross-over ~ 3500) */
    int32_t host_eig_threads;    /* helper threads of the host K x K eigensolver's rotation replay (default 0:
                                  * measured slower on the MI355X host; results are bit-identical) */
    int32_t block_threads;       /* host threads for several eigensolver-sized PSD blocks: worker threads driving per-block
                                  * streams (blocks that are not batched) and the helper threads of a batched run's
                                  * per-block restart logic (they spin only while a batched projection is in progress):
                                  * -1 auto = min(8, blocks), 0 = none (blocks / restart logic in sequence) */
    int32_t host_eig_merge;      /* K x K Rayleigh-quotient eigensolve of the thick-restart Lanczos by SPLIT + RANK-ONE MERGE
                                  * (csrc/host_eig_merge.hpp: the arrow part / first half is decomposed while the GPU still
                                  * runs the cycle -- its coefficients are read back early on a side stream -- and only the
                                  * small tail + one secular-equation merge stay on the critical path; only the Ritz vectors
                                  * actually needed are formed): -1 auto = from krylovdim 64 on, 0 = implicit QL always,
                                  * 1 = from krylovdim 24 on.  Same decomposition to rounding (orthogonality ~1e-14). */
    int32_t block_batch;         /* PSD blocks of EQUAL side whose projections take the Krylov branch (KrylovKit mode,
                                  * packed-triangle operator, krylovdim <= 63) advance their Lanczos recurrences in ONE
                                  * launch per step (grid.z = block; groups of up to 8) instead of one stream + host thread
                                  * per block: -1 auto = 1 = on, 0 = off.  Per block the arithmetic is unchanged. */
    int32_t rocsolver_warmup;    /* 1 = load rocSOLVER's code objects from a background thread at start-up (default 0) */
    int32_t debug_fail_iteration;/* k > 0: FAULT INJECTION for tests -- this process throws inside the PSD projection of
                                  * iteration k (a block-sharded solve must then abort on EVERY shard after that
                                  * iteration's scalar reduce instead of leaving the peers in a collective); 0 = never.
                                  * Honoured only when PROXSDP_HIP_FAULT_INJECTION=1 is set in the environment as well
                                  * (otherwise PROXSDP_E_INVALID): a test switch, not a user option.  In a call of
                                  * proxsdp_hip_solve_sharded with several shards it applies to the LAST shard only */
    int32_t host_wait_spin;      /* how the solver thread waits for the GPU at its per-cycle / per-iteration read-backs:
                                  * 1 = poll hipStreamQuery (no sleep: the wake-up of a blocked wait costs tens of
                                  * microseconds per synchronisation and leaves the core cold for the K x K eigensolve
                                  * that follows), 0 = hipStreamSynchronize, -1 auto = 1 */
    int32_t sign_start_row;      /* sign-function projection: row of the coefficient table the iteration starts at.  The
                                  * table resolves |eigenvalues| down to 1e-10 x the spectral scale in 19 steps; the
                                  * iterates of a solve rarely come closer to singular than 1e-5, so the iteration starts
                                  * further down the table, TESTS the result (sum t^2 (1 - t^2) over the eigenvalues t of
                                  * the computed sign matrix, from two Frobenius norms) and continues with the rows it
                                  * skipped only when the test fails -- same error bound either way.
                                  * -1 auto: adaptive per block (starts at row 8: 34 products instead of 57; a failure
                                  * sends the next 8 projections two rows down, a second one soon after lowers the row for good); 0 = the full table, no test
                                  * (round-2 behaviour); k > 0 = always start at row k (capped where the test stops
                                  * resolving 1e-10) */
    int32_t general_batch;       /* linesearch candidates per read-back on every vector path (support set, full vectors,
                                  * dense M): -1 auto = 1 = up to 3 candidates, their residual and gap reductions in one
                                  * batch of launches and ONE read-back per iteration (the first the reference's loop would
                                  * accept wins); 0 = one candidate per read-back.  Per candidate the same arithmetic: the
                                  * same bits either way */
    int32_t full_eig_lanczos_certify; /* PER-CALL certificate of a Lanczos-served full_eig! (single-vector Lanczos shows one
                                  * eigenvector per distinct eigenvalue the start vector sees: a repeated positive eigenvalue
                                  * or a deficient start vector would drop positive pairs from X+): after convergence a
                                  * second, independent vector is orthogonalised against the returned Ritz vectors and run
                                  * through m steps of the same recurrence with them locked (Lanczos on the deflated
                                  * operator); its largest Ritz value must be <= full_eig_lanczos_posres x the spectral
                                  * scale, otherwise the dense engine projects that input.  -1 auto = 10 steps, 0 = off,
                                  * m >= 2 = m steps.  The periodic dense check (full_eig_lanczos_verify) stays behind it. */
    int32_t host_merge_threads;  /* helper threads for the rank-one merge of the K x K eigensolve (host_eig_merge): the secular
                                  * roots, the Gu-Eisenstat weights and the eigenvector columns are independent per root /
                                  * column and are handed out in chunks; the helpers spin only while a projection with
                                  * krylovdim >= 64 is in progress.  Results are bit-identical to the serial merge.
                                  * -1 auto = 3, 0 = none */
    int32_t reserved_i[1];       /* zero */
    double  full_eig_lanczos_tol;/* convergence of the POSITIVE Ritz pairs of that engine: residual <= tol x the spectral
                                  * scale; 0 (default) = krylovkit_tol as an absolute residual (KrylovKit's rule) */
    double  reserved_d[1];       /* zero */
    /* ---- ABI 9 (appended) ---- */
    int32_t equilibration_reference_aliasing; /* equilibrate! (equilibration.jl:1-72) builds `E = Diagonal(u)`, `D = Diagonal(v)`
                                  * WITHOUT copying (:16-17), so `E.diag .= exp.(u)` (:25-26) overwrites u with exp(u) (v with
                                  * exp(v)) at the top of every iteration and the gradient steps start from there.  1 (default):
                                  * that arithmetic, line by line -- what the reference computes; 0: the iteration the code
                                  * evidently intends (u, v kept; E = exp(u), D = exp(v)): rounds 1-4 behaviour */
    int32_t reserved_i3[2];      /* zero (two designs of round 5 -- a device-side thick restart and a warm-started block filter for the
                                  * Lanczos-served full_eig! -- were measured out before they got an option: DESIGN.md section 9) */
    int32_t block_batch_groups;  /* batched multi-block Lanczos (block_batch): equal-side blocks are split into this many groups that
                                  * run CONCURRENTLY (own stream + host thread each): one group's restart logic on the host overlaps
                                  * the other groups' cycles on the GPU.  -1 auto = 1 = groups run ONE AFTER THE OTHER (rounds 3-4 behaviour; also when more than 8 equal-side
                                  * blocks force several groups), k >= 2 = k
                                  * groups (from 4 blocks on, when the block worker pool is up: block_threads != 0).  Per block
                                  * nothing changes.  MEASURED NEGATIVE on MIMO 8 x 513 (same session: 313 / 303 / 217 it/s with
                                  * 1 / 2 / 4 groups): a cycle is bound by its chain of dependent launches on the GPU (135 us of
                                  * the 200), kernels of different streams do not overlap enough to pay for twice the launches --
                                  * kept as an opt-in for models with many more blocks */
    int32_t lanczos_wide_krylov; /* Krylov dimensions 256..511 (target rank up to 255, eigsolver_min_lanczos up to 511): 0 (default) =
                                  * the dense eigensolver serves those projections (dense_truncated_projections); 1 = the
                                  * wide Lanczos kernels run them on the device (KrylovKit's thick restart, as for the narrow
                                  * dimensions; wide_krylov_projections counts them).  Larger dimensions stay dense either way.
                                  * The workspace is wide only for a block whose max(2 max_target_rank_krylov_eigs + 1,
                                  * eigsolver_min_lanczos) exceeds 255.  Other values: PROXSDP_E_INVALID */
    int32_t reserved_i2[6];      /* zero */
    int32_t device_eig_merge;    /* (the last reserved_i2 slot: reserved_i2 keeps its offset)  the rank-one merge of the split
                                  * K x K eigensolve (host_eig_merge) on the DEVICE (csrc/merge_device.hip.hpp): the host keeps the
                                  * two QL decompositions and the deflation plan; secular roots, Gu-Eisenstat weights, the
                                  * eigenvector product and the coefficients of the restart rotation are five short launches
                                  * and never visit the host.  -1 auto = on for the step kernels wherever the split runs with a
                                  * Krylov dimension >= 64, 0 = off (the merge stays on the host), 1 = on wherever the split
                                  * runs (with host_eig_merge = 1 from Krylov dimension 24 on).  Wide, batched and one-workgroup
                                  * runs and block worker threads keep the host merge; a merge the device hands back (a root at
                                  * the iteration cap, a non-finite value) or could not take is counted in
                                  * device_eig_merge_fallbacks and redone on the host. */
    double  full_eig_lanczos_warm_pow; /* start vector of a Lanczos-served full_eig! (positive-part run, the library's own engine): the
                                  * previous projection's Ritz vectors are summed with weights (lam_0 / lam_c)^p -- the pairs with the SMALL
                                  * eigenvalues are the ones such a run converges last, so they get the larger share.  Default 1.0
                                  * (measured, default-options solves: n = 4000: 687 201 -> 666 808 mat-vecs, 11.3-11.4 -> 10.9-11.1 s; n = 2000:
                                  * 323 250 -> 316 127; n = 3000: 492 988 -> 486 157; the same iteration counts and objectives; every p in
                                  * 0.125 .. 3 tried was better than 0); 0 = the plain sum of rounds 3-4 */
    double  reserved_d2[3];      /* zero */
} proxsdp_options;

#define PROXSDP_TRACE_COLS 14
/* trace row: iter, prim_obj, dual_obj, gap, feas, prim_res, dual_res, primal_step,
 *            beta, theta, target_rank(block 0), linesearch trials,
 *            elapsed (s since the loop started, host clock after the iteration's last
 *            stream synchronisation), Lanczos mat-vecs of this iteration */

/* counters and timers (the reference's TimerOutputs sections) */
typedef struct proxsdp_stats {
    int64_t lanczos_matvecs;     /* symmetric mat-vecs inside Lanczos (all blocks)   */
    int64_t lanczos_restarts;
    int64_t lanczos_calls;
    int64_t full_eigs;           /* full_eig! calls                                  */
    int64_t krylov_fallbacks;    /* Krylov not converged -> full_eig! fallback       */
    int64_t linesearch_trials;
    int64_t symv_launches;       /* == lanczos_matvecs                               */
    int64_t symv_profiled;       /* launches bracketed by events                     */
    double  symv_profiled_ms;    /* sum of their durations                           */
    double  symv_bytes;          /* algorithmic bytes of all symv launches (8*N + 16*n each) */
    double  algorithmic_bytes;   /* B_iter summed over iterations        */
    double  init_time;           /* s: preprocess + upload ("Init")                  */
    double  loop_time;           /* s: the PDHG loop ("CP loop")                     */
    double  exit_time;           /* s: cache_solution                                */
    double  t_primal, t_psd, t_linesearch, t_residual;   /* s, host wall incl. syncs: the reference's TimerOutputs sections (pdhg.jl:150-164).
                                  * t_primal = primal_step! incl. the projection (t_psd); on every path the residual / gap REDUCTIONS
                                  * ride in the linesearch candidates' batch and its read-back (counted in t_linesearch), t_residual is
                                  * what is left of compute_residual! / compute_gap!: the host scalars */
    int64_t dense_passes;        /* passes over a dense A (A x or batched A' y), 8*p*n bytes each */
    double  dense_ms;            /* their summed durations (HIP events on the solve stream)    */
    int64_t fop_projections;     /* projections whose Lanczos mat-vecs ran in operator form     */
    int64_t exit_matvecs;        /* mat-vecs of the exit path's lambda_min(dual cone) Lanczos   */
    double  host_eig_time;       /* s: K x K Rayleigh-quotient eigensolves done on the HOST     */
    int64_t host_eigs;           /* how many of them                                            */
    int64_t device_eigs;         /* unused (0): a device-side K x K eigensolver was measured and dropped, DESIGN.md section 9 */
    int64_t batched_small_eigs;  /* small-block (n <= 32) projections done by the batched Jacobi kernel */
    int64_t mfma_reconstructions;/* reconstructions that took the MFMA (v_mfma_f64_16x16x4) SYRK */
    int64_t orth_profiled;       /* k_lz_orth launches bracketed by events (profile_symv_every)  */
    double  orth_profiled_ms;    /* sum of their durations                                       */
    double  full_eig_solver_ms;  /* full_eig!: dense eigensolver time (events; profile_symv_every > 0) */
    double  full_eig_recon_ms;   /* full_eig!: reconstruction kernel time (events)               */
    int64_t cycle_launches;      /* Lanczos cycles run by the one-workgroup kernel (lanczos_cycle_kernel = 2) */
    int64_t full_eigs_lanczos;   /* full_eig! calls served by the Lanczos engine (all positive pairs) */
    int64_t cycle_steps;         /* Lanczos steps run inside those launches                       */
    double  cycle_ms;            /* their summed kernel time (events; profile_symv_every > 0)     */
    int64_t warm_starts;         /* projections started from the previous Ritz vectors (lanczos_warm_start) */
    int64_t full_eigs_sign;      /* full_eig! calls served by the sign-function projection (full_eig_sign) */
    int64_t sign_products;       /* symmetric n x n matrix products (fp64 MFMA) those calls took */
    int64_t sign_engine_projections; /* Krylov-branch projections served by the sign function (psd_sign_engine) */
    int64_t sign_engine_rejected;    /* ... computed but discarded: truncation was active, Lanczos redid them */
    int64_t sign_engine_checks;      /* verification rounds (both engines on the same input; first use, then every 64th) */
    int64_t sign_engine_mismatches;  /* ... that disagreed (repeated eigenvalues): the block stays with Lanczos */
    int64_t full_eigs_lanczos_checks;     /* Lanczos-served full_eig! calls verified against the dense engine */
    int64_t full_eigs_lanczos_mismatches; /* ... that disagreed: the block went back to the dense engine */
    int64_t batched_block_steps;     /* Lanczos steps launched for several blocks at once (block_batch) */
    int64_t rccl_reductions;         /* collectives issued by the library itself on its own stream (nccl_comm) */
    int64_t batched_profiled_blocks; /* block mat-vecs inside the event-bracketed batched launches (symv_profiled
                                      * counts launches; bytes of those launches = this x (8 N + 16 n)) */
    int64_t host_eig_merges;         /* K x K eigensolves done by split + rank-one merge (host_eig_merge); host_eig_time
                                      * then counts only their critical-path part */
    double  host_eig_overlap_time;   /* s: the part of those eigensolves done while the GPU was running the cycle */
    int64_t sign_short_pass;         /* sign-function projections whose shortened schedule passed its test (sign_start_row) */
    int64_t sign_short_fail;         /* ... that failed it and continued with the skipped rows */
    int64_t full_eigs_lanczos_certified;  /* Lanczos-served full_eig! calls whose certificate run passed (full_eig_lanczos_certify) */
    int64_t full_eigs_lanczos_cert_failed;/* ... whose certificate found a positive direction outside the returned pairs: the
                                           * dense engine projected that input instead */
    int64_t cert_matvecs;                 /* mat-vecs of those certificate runs (included in lanczos_matvecs) */
    /* ---- ABI 9 (appended) ---- */
    int64_t dense_truncated_projections;  /* Krylov-branch projections whose krylovdim = max(2 target_rank + 1, eigsolver_min_lanczos)
                                           * exceeds the step kernels' 255 columns: served by the dense eigensolver (top target_rank
                                           * pairs of dsyevd, the same truncated projection and min_eig); status_string says so */
    int64_t wide_krylov_projections;      /* Krylov-branch projections with a Krylov dimension of 256..511 run by the wide Lanczos
                                           * kernels (lanczos_wide_krylov = 1) */
    int64_t reserved_s[4];                /* [0] = sharded_general_iterations (PROXSDP_STATS_SHARDED_GENERAL_ITERATIONS below):
                                           * iterations a block-sharded solve ran on the general vector path on THIS shard (a
                                           * shard with an SOC, a 1x1 PSD block or no PSD block; 0 on a support-path shard and
                                           * in a solve that is not sharded); [1] = device_eig_merges: merges of host_eig_merges
                                           * whose O(k^2) part ran on the device (device_eig_merge); [2] = device_eig_merge_fallbacks:
                                           * merges the host did while the device path was switched on (a shape or a thread it does
                                           * not serve, or a merge it handed back); [3] = fop_owner_steps: k_lz_orth launches of the
                                           * operator-form Lanczos step that read t = Vp'v finished by the mat-vec launch's
                                           * column owners (environment PROXSDP_HIP_FOP_OWNER = 0: never; unset: where it applies) */
    /* (the last two reserved slots: reserved_s keeps its offset) */
    int64_t dense_setup_passes;           /* set-up passes over a dense A (row sums + extrema, 8*p*n bytes): 1 when equilibration
                                           * was asked for, else 0 */
    int64_t dense_sigma_steps;            /* Lanczos steps of the device sigma_max (approx_norm = 0 with a dense A): two passes
                                           * over the dense A each, counted in dense_passes / dense_ms as well */
} proxsdp_stats;
/* named slots of proxsdp_stats.reserved_s (the array keeps its four slots and its offset; a slot that gets a meaning keeps its place) */
#define PROXSDP_STATS_SHARDED_GENERAL_ITERATIONS 0
#define PROXSDP_STATS_DEVICE_EIG_MERGES 1
#define PROXSDP_STATS_DEVICE_EIG_MERGE_FALLBACKS 2
#define PROXSDP_STATS_FOP_OWNER_STEPS 3

/* Result (structs.jl:60-81).  Arrays are caller-allocated with the stated
 * lengths (NULL = not wanted); values are unscaled and in USER variable order
 * (pdhg.jl:768-769).  objval/dual_objval are the minimisation objective; the
 * sign/constant fix-up of MOI_wrapper.jl:336-337 stays with the caller. */
typedef struct proxsdp_result {
    int32_t status;                 /* PROXSDP_STATUS_*                              */
    int32_t certificate_found;
    int32_t primal_feasible_user_tol;
    int32_t dual_feasible_user_tol;
    int32_t result_count;
    int32_t final_rank;
    int64_t iter;
    double  primal_residual;        /* carries equa_feasibility (sic, pdhg.jl:774)   */
    double  dual_residual;          /* carries ineq_feasibility (sic, pdhg.jl:775)   */
    double  objval, dual_objval, gap, time;
    double  dual_feasibility;       /* value behind dual_feasible_user_tol           */
    double* primal;                 /* n */
    double* dual_cone;              /* n */
    double* dual_eq;                /* p */
    double* dual_in;                /* m */
    double* slack_eq;               /* p */
    double* slack_in;               /* m */
    double* trace;                  /* trace_capacity x PROXSDP_TRACE_COLS, row-major */
    int64_t trace_rows;             /* rows written                                  */
    char    status_string[256];
    proxsdp_stats stats;
} proxsdp_result;

/* State of a solve at an ITERATION BOUNDARY (after iteration `iteration`'s control logic, pdhg.jl:246-483, before
 * primal_step! of the next one): everything chambolle_pock carries from one iteration to the next.  At that point
 * x_old = x, y_old = y, Mty_old = Mty, Mx_old = Mx (residuals.jl:65-68), so four vectors suffice.  Vectors are in the
 * solver's INTERNAL order and scaling (preprocess! + norm_scaling, scaling.jl:2-49: cone variables first, PSD
 * off-diagonals carrying sqrt(2)).  Test / measurement seam (oracle resume-from-state, steady-window baselines): the
 * eigensolver workspaces are not part of it -- the reference's KrylovKit start vector is fixed
 * (krylovkit_reset_resid = false) and the library's own caches (previous Ritz factors, engine statistics) are rebuilt.
 * Not available for block-sharded solves or with equilibration (PROXSDP_E_UNSUPP); an iteration inside a certificate
 * search (pdhg.jl:639-676) is not captured (ints[3] stays 0, the solve goes on). */
#define PROXSDP_STATE_NHIST 7
typedef struct proxsdp_state {
    int64_t struct_size;       /* = sizeof(proxsdp_state) */
    int64_t iteration;         /* capture: IN  the iteration to capture after (>= 1); resume: the iteration the state belongs to */
    int64_t n, Q, n_psd;       /* array lengths; must equal the problem's n, p + m, n_psd */
    int64_t hist_len;          /* = 2 * options.convergence_window */
    double* x;                 /* n */
    double* y;                 /* Q */
    double* Mty;               /* n */
    double* Mx;                /* Q */
    int64_t* target_rank;      /* n_psd (Params.target_rank, structs.jl:159-192) */
    int64_t* current_rank;     /* n_psd */
    double* min_eig;           /* n_psd */
    double* hist;              /* PROXSDP_STATE_NHIST x hist_len, raw circular storage (structs.jl:2-30: entry i at slot
                                * (i-1) mod hist_len): dual_gap | prim_obj | dual_obj | feasibility | primal_residual |
                                * dual_residual | comb_residual */
    double scal[16];           /* 0 primal_step 1 primal_step_old 2 dual_step 3 beta 4 theta 5 adapt_level
                                * 6 equa_feasibility 7 ineq_feasibility 8 dual_feasibility; rest zero */
    int64_t ints[8];           /* 0 rank_update 1 update_cont 2 ada_count (pdhg.jl:306-332) 3 OUT captured (1 = written);
                                * rest zero */
} proxsdp_state;

/* ------------------------------------------------------------------ drop-in */
int  proxsdp_hip_abi_version(void);
void proxsdp_hip_default_options(proxsdp_options* opt);          /* options.jl defaults */
/* set an option by its reference name (RawOptimizerAttribute semantics,
 * MOI_wrapper.jl:84-93): unknown name -> PROXSDP_E_INVALID */
int  proxsdp_hip_set_option(proxsdp_options* opt, const char* name, double value);
int  proxsdp_hip_get_option(const proxsdp_options* opt, const char* name, double* value);
/* replaces chambolle_pock(aff, con, opt) -- MOI_wrapper.jl:310, pdhg.jl:1-530 */
int  proxsdp_hip_solve(const proxsdp_problem* prob, const proxsdp_options* opt,
                       proxsdp_result* res);
/* the same solve with the state seam: `resume` (may be NULL) = continue from this state with iteration
 * resume->iteration + 1 instead of starting at pdhg.jl:54-142's initial point; `capture` (may be NULL) = write the state
 * after iteration capture->iteration into the caller-allocated arrays (capture->ints[3] = 1 when that iteration was
 * reached).  proxsdp_hip_solve(p, o, r) == proxsdp_hip_solve_ex(p, o, r, NULL, NULL). */
int  proxsdp_hip_solve_ex(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                          const proxsdp_state* resume, proxsdp_state* capture);
const char* proxsdp_hip_last_error(void);
int  proxsdp_hip_device_count(void);          /* <0: PROXSDP_E_HIP */

/* ------------------------------------------- block-sharded solve from ONE call
 * `prob` is the WHOLE model (either index base); the library splits it into n_shards shards itself, runs one shard per
 * host thread -- thread s on device device_ids[s] (repeats allowed; NULL = every shard on options.device_id) --, and returns
 * the whole model's result in the caller's order.  No process group, no communicator, no callback: the shards share one
 * in-process group (csrc/shard_group.hpp).  Per reduce every shard writes its packed [sums | maxs] record into its slot,
 * the shards meet at a barrier, and each combines the records in shard order (acc = rec[0]; acc += rec[r], r = 1, 2, ...;
 * element-wise maximum) -- the same bits on every shard.  The coupling rows of M x are summed by one kernel per shard that
 * reads every shard's partial buffer (peer access between the devices, enabled once; pinned host memory where a pair of
 * devices has none) and adds them in shard order.
 *   prob        must not itself be a shard: reduce_fn, reduce_vec_fn, nccl_comm or n_coupling != 0 give PROXSDP_E_INVALID;
 *               so does M_dense.  approx_norm = 0 and equilibration / equilibration_force != 0 give PROXSDP_E_UNSUPP.  There is
 *               no state seam.  eig_resid (optional) is split per cone.
 *   psd_owner / soc_owner / free_owner: shard of every PSD cone / SOC cone / variable outside every cone (ascending id), each
 *               may be NULL = ONE round-robin over the PSD cones, then the SOC cones, then the free variables.  A cone is
 *               never split.  An owner outside 0 .. n_shards - 1, a variable in two cones or a shard that would own no
 *               variable give PROXSDP_E_INVALID before any thread starts.
 *   rows        a row whose entries all lie in one shard's variables is private to it (a row without entries: shard 0); every
 *               other row is a coupling row, carried by all shards on their own columns and owned by the lowest shard that
 *               touches it.
 *   res         the whole model: primal, dual_cone (n), dual_eq, slack_eq (p), dual_in, slack_in (m) in user order -- a
 *               private row from its shard, a coupling row from its owner.  status, iter, objectives, gap, residuals,
 *               final_rank, time, status_string: the global values every shard agrees on (shard 0's copy).  Trace rows
 *               are shard 0's, except column 13 (mat-vecs: summed over the shards) and column 10 (the shard that holds the
 *               model's first PSD cone).  res->stats: counters, byte counts and the summed durations of profiled launches
 *               (*_ms) ADDED over the shards; the wall-clock timers (init_time, loop_time, exit_time, t_primal, t_psd,
 *               t_linesearch, t_residual, host_eig_time, host_eig_overlap_time) are the MAXIMUM over the shards.
 *   shard_stats n_shards entries (or NULL): every shard's own struct.
 * Inside the call the AUTO values of block_threads and host_merge_threads are divided among the shards (8 / n_shards worker
 * threads -- none below 2 -- and 3 / n_shards merge helpers per shard); explicit values are honoured.  Both knobs leave every
 * result bit-identical.  n_shards = 1 runs the plain solve's arithmetic.
 * The call never returns PROXSDP_E_COMM_ABORTED, and no barrier of the group hangs: a shard that leaves the solve for any
 * reason wakes the others, a barrier wait longer than PROXSDP_HIP_COLLECTIVE_TIMEOUT_S seconds (default 300) abandons the
 * group, and a shard whose projection fails still joins that iteration's reduce, so that all shards stop after the same
 * iteration.  That bound covers the barriers ONLY, not the final join: before it frees its device buffers every shard waits,
 * without a deadline, until all shards have left the solve (a peer's coupling-sum kernel may still be reading them), and the
 * call joins all its threads.  A shard that is gone is noticed at once; a shard that is HUNG -- stuck inside a device call --
 * keeps the other shards and the call waiting for as long as it is stuck.  The return value
 * and proxsdp_hip_last_error() are those of the lowest shard that failed for reasons of its own; the text names the shard and
 * the iteration every shard stopped in. */
int  proxsdp_hip_solve_sharded(const proxsdp_problem* prob, const proxsdp_options* opt,
                               int32_t n_shards, const int32_t* device_ids,
                               const int32_t* psd_owner, const int32_t* soc_owner, const int32_t* free_owner,
                               proxsdp_result* res, proxsdp_stats* shard_stats);

/* ------------------------------------------- the solve, with the low-rank factors of its PSD solution
 * The projection computes the PSD iterate as X = V Lam+ V' from r Ritz pairs (prox_operators.jl:89-109) and the reference
 * returns only the matrix (Result.primal): a caller who needs the factor -- Goemans-Williamson rounding, sensor positions, a
 * rank-one symbol vector -- pays a dense eigendecomposition of what was just built from it.  This entry hands the factor out.
 * The solve is proxsdp_hip_solve's, bit for bit (iterates, counts, res, stats other than exit_time); the factors are taken
 * at the snapshot that fills res (the last one when a certificate search takes several), from the block exactly as it is
 * returned in res->primal -- res->primal itself may be NULL.  Cones in the caller's cone order; a PSD cone's variable list
 * is its upper triangle column by column, so row i of V is row i of the matrix.
 *   cap[k]      columns the caller has room for; 0 = nothing wanted for cone k: nothing is computed or written for it (rank,
 *               rank_found, source, resid, xnorm = 0)
 *   vectors     cone k at vectors + vec_ptr[k]: side_k x rank[k], column-major, ld = side_k; values at values + val_ptr[k]:
 *               rank[k] eigenvalues, descending, all > 0.  When rank_found[k] > cap[k] the cap[k] largest pairs are written
 *   source      PROXSDP_FACTOR_RITZ: the Ritz pairs of the last projection (the block is still their reconstruction: the
 *               Krylov branch, a Lanczos-served full_eig!, not equilibrated) -- one gather and one 8 side rank byte
 *               download, no eigensolve, accurate to the reconstruction's rounding, orthonormal to what the Lanczos run
 *               left (krylovkit_tol);  PROXSDP_FACTOR_EIG: one dsyevd of the final block, pairs with lambda > 0 kept (the
 *               other full_eig! engines, equilibrated solves, a snapshot inside a certificate search before the next
 *               projection);  PROXSDP_FACTOR_NONE: a 1x1 cone (V = [1], lambda = x when x > 0, else rank 0)
 *   resid       ||X_k - V diag(values) V'||_F of what was written against the returned block, xnorm = ||X_k||_F, both over
 *               the full symmetric matrix (off-diagonals count twice), computed on the device (k_factor_residual); with
 *               rank_found[k] > cap[k] resid reports what was cut
 * PROXSDP_E_INVALID before any device call: fac NULL, a wrong struct_size, n_psd != prob->n_psd, a NULL array (vectors /
 * values may be NULL only when no cone asks for a column), a negative cap, a vec_ptr / val_ptr span smaller than
 * side_k cap[k] / cap[k] (cap counted up to side_k: a block has no more pairs).  PROXSDP_E_UNSUPP: prob is a shard
 * (reduce_fn, reduce_vec_fn, nccl_comm, n_coupling != 0).  proxsdp_hip_solve_sharded and the state seam have no such variant. */
#define PROXSDP_FACTOR_NONE 0
#define PROXSDP_FACTOR_RITZ 1
#define PROXSDP_FACTOR_EIG  2
typedef struct proxsdp_psd_factors {
    int64_t struct_size;     /* = sizeof(proxsdp_psd_factors) */
    int64_t n_psd;           /* IN: must equal prob->n_psd */
    const int64_t* cap;      /* IN  n_psd: columns available for cone k (0 = none wanted for it) */
    const int64_t* vec_ptr;  /* IN  n_psd+1: offsets into vectors; vec_ptr[k+1]-vec_ptr[k] >= side_k*cap[k] */
    const int64_t* val_ptr;  /* IN  n_psd+1: offsets into values;  >= cap[k] */
    double*  vectors;        /* OUT cone k: side_k x rank[k], column-major, ld = side_k */
    double*  values;         /* OUT cone k: rank[k] eigenvalues, DESCENDING, all > 0 */
    int64_t* rank;           /* OUT n_psd: columns written = min(cap[k], rank_found[k]) */
    int64_t* rank_found;     /* OUT n_psd: positive pairs the block has */
    int32_t* source;         /* OUT n_psd: PROXSDP_FACTOR_* */
    double*  resid;          /* OUT n_psd: ||X_k - V diag(lam) V'||_F, X_k = the block as returned in res->primal */
    double*  xnorm;          /* OUT n_psd: ||X_k||_F */
} proxsdp_psd_factors;
int  proxsdp_hip_solve_factored(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                                proxsdp_psd_factors* fac);

/* ------------------------------------------- warm start: the solve, entered from a point the caller gives
 * Every other entry starts at x = 0 (or tau c, advanced_initialization), y = 0, as the reference does (its warm start is a
 * stub: MOI_wrapper.jl:302).  This one enters proxsdp_hip_solve's loop at iteration 1 from the caller's point, given in the
 * units a result comes back in, so a previous result -- and the factors proxsdp_hip_solve_factored handed out -- can be fed
 * straight back:
 *   internal x  = primal gathered into the solver's order, off-diagonal PSD entries x sqrt(2), divided by D in an equilibrated
 *                 solve; internal y = [dual_eq; dual_in] divided by E: the inverse of what fills a result (cache_solution,
 *                 pdhg.jl:745-787), entry by entry on the device (k_start_gather)
 *   rank[k] >= 0  cone k starts at V diag(values) V', built by the solver's own reconstruction kernel straight into the
 *                 iterate (no packed triangle crosses the host); the entries of `primal` for that cone are ignored;
 *                 rank[k] = 0 is a zero block; rank[k] = -1: no factors for this cone (its entries come from `primal`)
 *   primal NULL   every variable outside a factored cone keeps its cold value (tau c under advanced_initialization, else 0)
 *   M x and M'y of the point come from the solver's own product launches; x_old, y_old, (M x)_old, (M'y)_old equal the
 *   current vectors; history, rank_update, update_cont, ada_count, current_rank, min_eig and theta start as in a cold solve.
 *   The point is NOT projected: the first iteration's primal step does that.
 *   target rank of cone k: target_rank[k] > 0 wins (capped at the side); otherwise, with factors for the cone,
 *                 min(side, max(initial_target_rank, rank[k] + 1)) -- the projection then sees the first non-positive
 *                 eigenvalue and the rank test passes at once; otherwise initial_target_rank.  A start pays only with the
 *                 right target rank: at the cold default of 2 the first projection truncates the point.
 *   primal_step, beta: 0 = the cold values (1 / norm(M), initial_beta); dual_step = primal_step as in a cold solve.
 * A start that gives no point at all (primal, dual_eq, dual_in NULL and no cone with rank >= 0) leaves the cold vectors as
 * they are (x_old = 0): with target_rank, primal_step and beta at 0 as well that is proxsdp_hip_solve bit for bit, as is
 * start == NULL.  fac != NULL additionally returns the factors as proxsdp_hip_solve_factored does, so solves chain.
 * PROXSDP_E_INVALID before any device call: a wrong struct_size; n_psd neither 0 nor prob->n_psd; a NULL rank / vec_ptr /
 * val_ptr with n_psd != 0; rank[k] < -1 or > side_k; a vec_ptr / val_ptr span smaller than side_k rank[k] / rank[k]; NULL
 * vectors / values while some rank[k] > 0; a non-finite entry anywhere; a value <= 0; a negative target_rank, primal_step or
 * beta; (fac: as proxsdp_hip_solve_factored).  PROXSDP_E_UNSUPP: prob is a shard (reduce_fn, reduce_vec_fn, nccl_comm,
 * n_coupling != 0).  There is no sharded variant and no combination with the state seam. */
typedef struct proxsdp_start {
    int64_t struct_size;       /* = sizeof(proxsdp_start) */
    const double* primal;      /* n, caller's variable order and scale (what res->primal holds), or NULL */
    const double* dual_eq;     /* p, as res->dual_eq, or NULL (= 0) */
    const double* dual_in;     /* m, as res->dual_in, or NULL (= 0) */
    int64_t n_psd;             /* 0 = no factors given; otherwise must equal prob->n_psd */
    const int64_t* rank;       /* n_psd: columns given for cone k; -1 = no factors for this cone */
    const int64_t* vec_ptr;    /* n_psd+1 offsets into vectors, as in proxsdp_psd_factors */
    const int64_t* val_ptr;    /* n_psd+1 offsets into values */
    const double* vectors;     /* cone k: side_k x rank[k], column-major, ld = side_k */
    const double* values;      /* rank[k] values, all finite and > 0 (any order; V need not be orthonormal) */
    const int64_t* target_rank;/* n_psd or NULL; entry 0 = derive (above) */
    double primal_step, beta;  /* 0 = the cold values */
} proxsdp_start;
int  proxsdp_hip_solve_from(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                            const proxsdp_start* start, proxsdp_psd_factors* fac /* may be NULL */);
/* test entry: the "Init" section and the start path of proxsdp_hip_solve_from, nothing more.  Writes the internal x, Mty (n),
 * y, Mx (Q), target_rank (n_psd), scal[0..5] and iteration = 0 into the caller-allocated `out` (struct_size, n, Q, n_psd must
 * match; current_rank, min_eig, hist and hist_len are not touched).  Unlike the state seam it is served with equilibration
 * and with a dense A.  start may be NULL (the cold point). */
int  proxsdp_hip_start_point(const proxsdp_problem* prob, const proxsdp_options* opt, const proxsdp_start* start,
                             proxsdp_state* out);

/* ------------------------------------------- solution vectors on the device: out of a solve, and back into the next
 * proxsdp_hip_solve_device is proxsdp_hip_solve_from bit for bit -- iterates, counts, trace, res, factors -- with two
 * differences in where vectors live:
 *   out_dev    the six solution vectors are written into DEVICE buffers of the caller, in the caller's variable order and in
 *              the units a result holds: exactly the values res->primal ... res->slack_in would hold.  A NULL member is not
 *              wanted.  Host arrays in `res` may be given as well; they receive the same values, each as ONE contiguous
 *              download of the vector the device formed.
 *   start_dev  primal, dual_eq and dual_in of the start point as DEVICE buffers, in the units a result holds (so out_dev of one
 *              solve is start_dev of the next); k_start_gather reads them where they are, no host copy and no upload.  Factors,
 *              target_rank, primal_step and beta still come from `start` (they are small).  dual_cone, slack_eq and slack_in
 *              must be NULL here.
 * The exit path of this entry runs on the device (csrc/exit_device.hip.hpp, Solver::cache_solution_device): M x, c + M'y, the
 * slacks, the scatter to the caller's order and the cone reductions of the dual feasibility are kernels compiled with
 * floating-point contraction off, every sum in the host path's order, so every output equals proxsdp_hip_solve_from's bit for
 * bit; the iterate never visits the host.  stats.exit_time is that path's time.
 * Device pointers are BORROWED and TRUSTED, exactly as M_dense with M_dense_on_device = 1 is: they must be valid on device
 * options.device_id for n / p / m doubles, must not overlap each other, and are not probed.  The library works on a stream of
 * its own: the caller finishes its own work on the buffers before the call (a device synchronisation, or its streams'), and
 * the call returns after every write has completed (it synchronises its stream).  There is no stream argument.
 * PROXSDP_E_INVALID on the host, before any device call: a wrong struct_size; device_id != options.device_id; a non-NULL
 * dual_cone, slack_eq or slack_in in start_dev; a vector given both in `start` and in `start_dev`; everything
 * proxsdp_hip_solve_from refuses.  ONE check happens after the device exists: that primal, dual_eq and dual_in of start_dev
 * hold finite numbers is a reduction on the device after set-up; a non-finite entry returns PROXSDP_E_INVALID before
 * iteration 1, and the message names the vector.  PROXSDP_E_UNSUPP: prob is a shard (as proxsdp_hip_solve_factored).
 * With start, start_dev, fac and out_dev all NULL the call is proxsdp_hip_solve_from with the device exit path. */
typedef struct proxsdp_device_vectors {
    int64_t struct_size;    /* = sizeof(proxsdp_device_vectors) */
    int32_t device_id;      /* must equal options.device_id */
    int32_t reserved;
    double* primal;  double* dual_cone;      /* n each,  DEVICE pointers, NULL = not wanted / not given */
    double* dual_eq; double* slack_eq;       /* p each */
    double* dual_in; double* slack_in;       /* m each */
} proxsdp_device_vectors;
int  proxsdp_hip_solve_device(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_result* res,
                              const proxsdp_start* start /* may be NULL */, const proxsdp_device_vectors* start_dev /* may be NULL */,
                              proxsdp_psd_factors* fac /* may be NULL */, proxsdp_device_vectors* out_dev /* may be NULL */);
/* ------------------------------------------- a model that stays on the device between solves: handle, updates, re-solve
 * No call of the reference stands behind this section: ProxSDP rebuilds AffineSets, ConicSets, the operator and every
 * workspace in each optimize! (/root/reference/src/MOI_wrapper.jl:220-342).  A handle does that work ONCE:
 *   create   everything proxsdp_hip_solve_device does before its first step size -- validation, variable order, scaling, the
 *            operator in both orientations, block classification, workspaces, support set, ELL structures, candidates, the
 *            device exit path's arrays -- and copies what it needs: no pointer of `prob` (eig_resid included) is used after
 *            it returns.  Every argument check of proxsdp_hip_solve applies, with the same codes and texts.  Equilibration
 *            and approx_norm = 0 are served as proxsdp_hip_solve serves them.  PROXSDP_E_UNSUPP, decided on the host before
 *            any device call: prob is a shard of a block-sharded solve; M_dense != NULL (the matrix is borrowed, a handle
 *            would outlive the loan); options.rocsolver_warmup != 0.
 *   solve    proxsdp_hip_solve_device on the model's current data, BIT FOR BIT -- iterates, iteration and trial counts,
 *            trace, res, factors, the six vectors, every counter of stats -- on the first solve of a handle and on every later
 *            one, whatever ran on the handle before.  Only the clocks differ (res->time, trace column 12, the *_time, t_* and
 *            *_ms members of stats): res->time and options.time_limit count from the entry into proxsdp_hip_model_solve,
 *            stats.init_time is what this solve spent before iteration 1 (the reset and the start path).  start, start_dev,
 *            fac and out_dev are checked as proxsdp_hip_solve_device checks them, against the model's dimensions and cones.
 *            run_opt = NULL: the options of create.  Otherwise every field must equal create's except time_limit, max_iter,
 *            log_verbose, log_freq, warn_on_limit and trace_capacity, which shape nothing in the set-up; a difference in any
 *            other field (the tolerances included: small_block_batch and full_eig_sign read them in auto mode) returns
 *            PROXSDP_E_INVALID and names the field.  A solve that fails -- a non-finite device start (PROXSDP_E_INVALID
 *            before iteration 1), an error out of the loop -- or stops at its time limit leaves the handle usable: the next
 *            solve is again the fresh solve bit for bit.  The block workers and the merge helpers are started per solve and
 *            joined at its end: a handle holds no thread between calls.
 *   update   replaces data of the same shape (proxsdp_model_data): c, b, h in the caller's order, A_nzval / G_nzval in the
 *            storage order create() was given; the sparsity pattern stays; a NULL member is unchanged.  on_device = 0: host
 *            pointers; 1: DEVICE pointers on the model's device, borrowed and trusted as proxsdp_device_vectors are (finish
 *            your own work on them before the call; the call returns after its reads have completed).
 *            PROXSDP_E_INVALID on the host: a NULL handle, a wrong struct_size, every pointer NULL.  Non-finite values are
 *            refused (PROXSDP_E_INVALID) before anything is written -- host arrays by a host loop, device arrays by a
 *            reduction on the device -- and the model keeps its previous data.  PROXSDP_E_UNSUPP: any update of an
 *            equilibrated model (E and D depend on the values); A_nzval / G_nzval with approx_norm = 0 (sigma_max depends on
 *            them).  The four scalars that feed the step size follow the data: ||b||, ||h||, ||c||, ||M||_F.
 *              host pointers    the host recomputes them in the order prepare() uses (the norms over the caller's arrays, the
 *                               Frobenius norm over the scaled values in reordered CSC order): a solve after a host update
 *                               EQUALS a fresh solve of the updated problem bit for bit.
 *              device pointers  they come from a device reduction in a fixed order (one partial per chunk of 4096 entries,
 *                               the partials added in chunk order by one thread): reproducible from run to run and
 *                               independent of the launch width, but NOT guaranteed equal to the host's last bit.
 *            An update of c may change which entries are zero and with them the support set {column non-empty or c_i != 0}
 *            of the support-aware vector path: the update then rebuilds what the set-up built from it (the auto rule may
 *            switch that path on or off, as it would in a fresh solve) and counts it in proxsdp_model_info.support_rebuilds.
 *   info     dimensions, counters, use_support, device_bytes (the handle's live device allocations), setup_time (seconds
 *            create took).
 *   destroy  frees everything; NULL is fine.
 * One handle serves one caller at a time. */
typedef struct proxsdp_model proxsdp_model;               /* opaque */
typedef struct proxsdp_model_data {
    int64_t struct_size;     /* = sizeof(proxsdp_model_data) */
    int32_t on_device;       /* 0: host pointers; 1: DEVICE pointers on the model's device, borrowed and trusted */
    int32_t reserved;
    const double* c;         /* n, caller's variable order, or NULL = unchanged */
    const double* b;         /* p */
    const double* h;         /* m */
    const double* A_nzval;   /* nnz(A) in the storage order create() was given; the pattern stays */
    const double* G_nzval;   /* nnz(G) */
} proxsdp_model_data;
typedef struct proxsdp_model_info {
    int64_t struct_size;     /* = sizeof(proxsdp_model_info) */
    int64_t n, p, m, n_psd, nnz;
    int32_t device_id;
    int32_t use_support;     /* 1: the support-aware vector path is on */
    int64_t solves, updates, support_rebuilds;
    int64_t device_bytes;
    double setup_time;
} proxsdp_model_info;
int  proxsdp_hip_model_create(const proxsdp_problem* prob, const proxsdp_options* opt /* NULL: defaults */, proxsdp_model** out);
int  proxsdp_hip_model_update(proxsdp_model* mdl, const proxsdp_model_data* upd);
int  proxsdp_hip_model_solve(proxsdp_model* mdl, const proxsdp_options* run_opt /* may be NULL */, proxsdp_result* res,
                             const proxsdp_start* start, const proxsdp_device_vectors* start_dev,
                             proxsdp_psd_factors* fac, proxsdp_device_vectors* out_dev);   /* the last four may be NULL */
int  proxsdp_hip_model_info(const proxsdp_model* mdl, proxsdp_model_info* info);
int  proxsdp_hip_model_destroy(proxsdp_model* mdl);       /* NULL is fine */
/* ------------------------------------------- inequality rows of a model handle added and dropped in place
 * The structural change of a cutting-plane loop: solve, separate violated inequalities, add them as rows of G x <= h, drop
 * the rows that went slack, re-solve from the previous point -- without destroy + create.  The reference has no counterpart
 * (it rebuilds everything per optimize!, as the section above says).
 *   G' = [the rows of G not in `drop`, in their old order; then the n_add new rows in the order given], h' likewise.
 * A, b, c and the cones are untouched; equality rows, new variables and new cones are out of scope.  m = 0 before and m' = 0
 * after are both valid; a new row may be empty; a new row may list a column twice (both stored entries are kept, as create
 * keeps duplicates).
 * STORAGE ORDER of G' -- the order a later proxsdp_hip_model_update(G_nzval) follows: column by column; inside a column its
 * kept entries in the order they are stored now, then its new entries by ascending new row; the entries of one row and
 * column in the order the row lists them.  For sorted, duplicate-free input this is the sorted CSC of the stacked matrix.
 * CONTRACT, the one every handle operation has: after the call proxsdp_hip_model_solve is proxsdp_hip_solve_device on the
 * problem with G', h' (stored in that order) BIT FOR BIT, and proxsdp_hip_model_dump equals the dump of a fresh model of it:
 * every decision a set-up derives from the matrix is taken again (the support path's auto rule, the wave-per-row mat-vec,
 * the long rows, the ELL structures of the operator form, general path versus support path).
 * The four norms follow the data as in update: on the host route (on_device = 0) ||h'|| and ||M'||_F are recomputed on the
 * host in prepare()'s order and equal a fresh model's to the last bit; on the device route they come from the fixed-order
 * device reduction update uses: reproducible, not guaranteed equal to the host's last bit.
 * What is rebuilt: everything sized by Q = p + m or by nnz -- y, M x and the candidates' y, [b; h], the operator's index and
 * value arrays in both orientations with its launch shapes, the exit path's value arrays and slack, the handle's position
 * maps -- and, ONLY when the set {column non-empty or c_i != 0} changed, the support set with what update rebuilds from it
 * (support_rebuilt = 1, counted in proxsdp_model_info.support_rebuilds).  What stays: everything sized by n or by a cone
 * side alone -- the Lanczos workspaces, the sign projection's work matrices, x and M'y, the small-block and SOC set-ups,
 * streams, events, the rocBLAS handle.  The values of kept entries do not visit the host on either route.
 * PROXSDP_E_INVALID, decided on the host before anything is written: a NULL handle; a wrong struct_size; n_drop and n_add
 * both 0 (or one negative); on_device other than 0 or 1; a NULL array that is needed; a drop number outside 0 .. m-1 or
 * repeated; add_ptr[0] != 0 or add_ptr not monotone; a column outside the model's variables; non-finite host values; Q' or
 * nnz' >= 2^31 (as create refuses them).  Device values are checked by a reduction on the device before anything is written;
 * the message names the array.  PROXSDP_E_UNSUPP: an equilibrated model (E and D depend on the rows); a model created with
 * approx_norm = 0 (sigma_max depends on them).  After a refused call the handle holds its previous data and solves as before.
 * ALLOCATION: every buffer of the new operator, of [b; h'], of the Q-sized vectors and of the maps is allocated BEFORE the
 * first write and before an old one is released: PROXSDP_E_NOMEM out of that phase leaves the old model in place.  The
 * segment lists of rows longer than 8192 entries and the support rebuild allocate after the new operator is in place; a
 * failure there leaves a handle that must be destroyed. */
typedef struct proxsdp_model_rows {
    int64_t struct_size;      /* = sizeof(proxsdp_model_rows) */
    int32_t on_device;        /* where add_val and add_h live: 0 host, 1 DEVICE pointers on the model's device, borrowed and
                               * trusted as proxsdp_model_data's are.  Index arrays are always HOST. */
    int32_t reserved;
    int64_t n_drop;  const int64_t* drop;     /* inequality rows to remove: 0-BASED numbers into the model's CURRENT G
                                               * (0 .. m-1), whatever index base, any order, no repeats */
    int64_t n_add;   const int64_t* add_ptr;  /* n_add + 1 offsets (0-based) into add_col / add_val: CSR of the new rows */
    const int64_t* add_col;                   /* variable numbers in the caller's numbering and the index base of create */
    const double*  add_val;                   /* host or device (on_device) */
    const double*  add_h;                     /* n_add right-hand sides, host or device (on_device) */
    /* out */
    int64_t m_new, nnz_new;
    int64_t* kept;            /* optional, caller-allocated, m - n_drop + n_add entries: new inequality row r was old row
                               * kept[r], -1 for an added row */
    int32_t support_rebuilt;  /* the support set or the vector path changed and was rebuilt */
    int32_t reserved2;
    int64_t bytes_allocated;  /* device bytes this call allocated (new buffers, whatever it freed) */
    double  seconds;          /* wall time of the call */
} proxsdp_model_rows;
int  proxsdp_hip_model_rows(proxsdp_model* mdl, proxsdp_model_rows* ch);
/* ------------------------------------------- separation on a model handle: violated triangle inequalities, slack rows
 * The other two verbs of the loop above.  The reference has no counterpart.
 * TRIANGLES.  For PSD cone `cone` of the handle (side s >= 3), X = the symmetric matrix of the cone's entries of `primal`
 * (n doubles, the caller's variable order, the units a result holds; the cone's variable list is its upper triangle, column
 * by column).  For 0 <= i < j < k < s and the patterns
 *     0: (-1, -1, -1)    1: (-1, +1, +1)    2: (+1, -1, +1)    3: (+1, +1, -1)
 * the inequality s1 X_ij + s2 X_ik + s3 X_jk <= rhs has the violation
 *     v = ((s1 * X_ij + s2 * X_ik) + s3 * X_jk) - rhs      fp64, left to right in this association, no contraction
 * (a product with +-1 is exact: any IEEE restatement gives the same bits).  The call returns the min(count, violated) rows
 * with the largest v among those with v > min_violation, ordered by v descending, equal v by (i, j, k, pattern) ascending;
 * that order also decides which rows of equal violation survive the cut-off.  `violated` counts ALL rows with
 * v > min_violation.  The result is a pure function of the inputs: the same rows and bits on every run, whatever the launch.
 * Outputs are HOST arrays, caller-allocated for `count` rows; entries past n_rows are not written.  add_col / add_val / add_h
 * with add_ptr = 0, 3, 6, ... are a proxsdp_model_rows change as they stand (add_col: the variables of X_ij, X_ik, X_jk in the
 * caller's numbering and the index base of create; add_val: the signs; add_h: rhs).
 * The handle's data is not touched: a solve after the call equals a solve before it bit for bit.  Scratch (the dense X of
 * 8 s^2 bytes, 2^12 counters, 16 cand_cap bytes of candidates) is allocated in the call, released before it returns and
 * reported in bytes_allocated, not in proxsdp_model_info.device_bytes; a host `primal` is expanded to X on the host.
 * How: a sweep over all C(s, 3) triples, once per pass of a radix select on the key (bits of v, then the index of
 * (i, j, k, pattern)) in digits of 12 bits -- a histogram pass per digit until at most cand_cap rows lie at or above the
 * prefix, then one pass that emits those; the host sorts them.  cand_cap = 0: max(4 count, 65536); a smaller value (at
 * least count is used) only forces more passes -- a test knob.
 * PROXSDP_E_INVALID, decided on the host before any device call: a NULL struct or handle; a wrong struct_size; on_device
 * other than 0 or 1; count < 1 or > 2^20; min_violation negative or not finite; rhs not finite; cand_cap < 0 or > 2^24; a
 * NULL primal; a NULL output array; a cone number outside the model; a cone of side < 3.  A non-finite entry of the cone's
 * part of primal: a host primal is checked by a host loop, a device primal by a reduction on the device before the sweep;
 * the message names the cone. */
typedef struct proxsdp_triangle_cuts {
    int64_t struct_size;      /* = sizeof(proxsdp_triangle_cuts) */
    int32_t on_device;        /* where primal lives: 0 host, 1 DEVICE pointer on the model's device, borrowed and trusted as
                               * proxsdp_model_data's are (proxsdp_host_triangle_cuts ignores it) */
    int32_t cone;             /* PSD cone of the model, 0-based in cone order (proxsdp_host_triangle_cuts ignores it) */
    int64_t count;            /* rows wanted: 1 .. 2^20 */
    double  min_violation;    /* >= 0 */
    double  rhs;
    int64_t cand_cap;         /* 0 = default; test knob */
    const double* primal;     /* n doubles (proxsdp_host_triangle_cuts ignores it: it is given X) */
    /* out: caller-allocated HOST arrays for `count` rows */
    int64_t* tri;             /* 3 per row: 0-based i < j < k */
    int32_t* pattern;
    double*  violation;
    int64_t* add_col;         /* 3 per row */
    double*  add_val;         /* 3 per row */
    double*  add_h;
    int64_t n_rows;           /* rows written: min(count, violated) */
    int64_t violated;         /* all rows with v > min_violation */
    int64_t scanned;          /* 4 C(s, 3) */
    int32_t passes;           /* sweeps over the triples (0 on the host) */
    int32_t reserved;
    int64_t bytes_allocated;  /* device bytes this call allocated (and released) */
    double  seconds;          /* wall time of the call */
    double  sweep_seconds;    /* the first sweep alone, between two device events */
} proxsdp_triangle_cuts;
int  proxsdp_hip_model_triangles(proxsdp_model* mdl, proxsdp_triangle_cuts* tc);
/* The same contract with no device and no handle: a serial enumeration with the expression above and a partial sort under the
 * same order.  X: the side x side matrix itself, row-major, symmetric, only i < j read.  cone_idx: the cone's variable list
 * (side (side + 1) / 2 numbers, upper triangle column by column) as add_col shall report it, or NULL = tri_index(i, j) +
 * index_base with tri_index(i, j) = j (j + 1) / 2 + i.  PROXSDP_E_INVALID: as above where it applies; NULL X; side < 3 or
 * > 46340; index_base other than 0 or 1; a non-finite X_ij, i < j. */
int  proxsdp_host_triangle_cuts(const double* X, int64_t side, const int64_t* cone_idx, int32_t index_base,
                                proxsdp_triangle_cuts* tc);
/* SLACK ROWS.  Given dual_in and slack_in of a result of the handle's current model (m doubles each, both host or both
 * device; slack_in = G x - h), the inequality rows r with |dual_in[r]| <= dual_tol and slack_in[r] < -slack_tol, as ascending
 * 0-based numbers in `rows` (HOST, caller-allocated, m entries; n_rows of them written): a `drop` list for
 * proxsdp_hip_model_rows.  A NaN in either vector fails its comparison: such a row is "not inactive"; it is not refused.
 * m = 0 gives 0 rows.  Device vectors are flagged and compacted by one kernel whose output order is the rows' own; its
 * scratch (8 m bytes) is released before the call returns.  PROXSDP_E_INVALID, on the host: a NULL struct, handle or array;
 * a wrong struct_size; on_device other than 0 or 1; a negative or non-finite tolerance. */
typedef struct proxsdp_inactive_rows {
    int64_t struct_size;      /* = sizeof(proxsdp_inactive_rows) */
    int32_t on_device;        /* dual_in and slack_in: 0 host, 1 DEVICE pointers on the model's device */
    int32_t reserved;
    const double* dual_in;    /* m */
    const double* slack_in;   /* m */
    double dual_tol, slack_tol;
    int64_t* rows;            /* out: HOST, m entries */
    int64_t n_rows;           /* out */
} proxsdp_inactive_rows;
int  proxsdp_hip_model_inactive_rows(proxsdp_model* mdl, proxsdp_inactive_rows* q);
/* ------------------------------------------- separation on a model handle: pentagonal and heptagonal cuts
 * Where the triangle rows stop biting, the odd-clique inequalities of the next sizes go on: for a +-1 vector x and signs
 * sigma on an odd set Q of k nodes the sum of sigma_a x_a is odd, its square at least 1, so
 *     sum over a < b in Q of  -sigma_a sigma_b X_ab  <=  (k - 1) / 2            (k = 3: the triangle rows above).
 * There are 16 C(s, 5) pentagonal rows: they are not enumerated.  The call GROWS given bases -- triangles (base_size q = 3)
 * into pentagons, pentagons (q = 5) into heptagons -- by the best pair of further nodes and their signs.  The reference has
 * no counterpart.
 * IN.   cone, primal, on_device: as in proxsdp_triangle_cuts (X is the same matrix).  n_base bases (1 .. 65536):
 *       base_nodes (n_base x q int64, 0-based nodes of the cone, strictly ascending inside a base) and base_sign (n_base x q
 *       int8, each +-1, the first of every base +1), both HOST arrays whatever on_device says.  rhs: finite ((q + 1) / 2, that
 *       is 2 and 3, for unit-diagonal models).  min_violation: finite, >= 0.
 * VALUE.  For a base with nodes a_0 < ... < a_{q-1} and signs sigma, two nodes l < m outside the base and tau_l, tau_m in
 *       {+1, -1}, in fp64, left to right exactly as written, no contraction (a product with +-1 is exact):
 *           B   = the sum over the pairs (u < w) of the base, in lexicographic order, of (-sigma_u sigma_w) * X[a_u, a_w],
 *                 starting from the first term
 *           t_l = ((sigma_0 * X[a_0, l] + sigma_1 * X[a_1, l]) + ...) + sigma_{q-1} * X[a_{q-1}, l]
 *           v   = (((B - tau_l * t_l) - tau_m * t_m) - (tau_l tau_m) * X[l, m]) - rhs
 * BEST.   The extension of a base is the (l, m, code) with the greatest v, equal v by the smallest (l, m, code); code = 0
 *       (+,+), 1 (+,-), 2 (-,+), 3 (-,-) for (tau_l, tau_m).  The base yields a row when that v > min_violation.
 * ROW.    The k = q + 2 nodes sorted ascending, the signs multiplied by the sign of the smallest node (one normal form per
 *       inequality).  Bases that yield the same (nodes, signs) are merged into the member with the greatest v, then the lowest
 *       base number.  Rows are ordered by v descending, then by that base number ascending.  At most n_base rows come back.
 * OUT (HOST arrays, caller-allocated for n_base rows; entries past n_rows are not written).  Per row: nodes (k), signs (k),
 *       violation, from_base, add_col / add_val (k (k - 1) / 2 = 10 or 21 entries in the lexicographic order of the pairs
 *       (u < w): the variable of X[n_u, n_w] in the caller's numbering and the index base of create, and -sigma'_u sigma'_w),
 *       add_h (= rhs): with add_ptr = 0, 10, 20, ... (or steps of 21) a proxsdp_model_rows change as they stand.  Per call:
 *       n_rows, violated_bases (bases that yielded a row, before merging), scanned = n_base 4 C(s - q, 2), bytes_allocated,
 *       seconds, sweep_seconds (the sweep kernels alone, between device events, summed over the batches).
 * The result is a pure function of the inputs: the same rows, order and bits on every run, whatever grid and batch are.  The
 * handle's data is not touched.  Scratch (the dense X of 8 s^2 bytes, 8 s min(n_base, batch) bytes of t rounded up to whole
 * waves of 64 bases, the bases, 16 bytes per (workgroup column, base) of partial results) is allocated in the call, released
 * before it returns and reported in bytes_allocated only.
 * How: k_tri_gather builds X; per batch of bases k_clique_rows writes t[l][base] (NaN at the base's own nodes: every later
 * comparison fails there) and B; k_clique_sweep gives a wave 64 bases, one per lane, and tiles of 64 x 64 pairs (l, m) of the
 * strict upper triangle -- X[l, m] is wave-uniform and read from LDS as a broadcast, t_m from LDS laid out [m][lane], t_l is
 * hoisted per l, the four codes are evaluated in order and each lane keeps its best (v, l, m, code) in registers; a workgroup
 * writes one partial best per (its range of tiles, base) and k_clique_best reduces them under the same total order, whose
 * maximum does not depend on how the tiles were split.  Merging, normal form, sort and the rows are the host's.
 * Test knobs (0 = the library's choice; the result does not depend on either): grid = workgroup columns of the sweep (each
 * owns a range of tiles), batch = bases per launch (rounded up to a multiple of 64; default 1024).
 * PROXSDP_E_INVALID, decided on the host before any device call, the message naming the field: a NULL struct, handle or
 * array; a wrong struct_size; on_device other than 0 or 1; base_size not 3 or 5; n_base outside 1 .. 65536; a cone outside
 * the model; a cone of side < q + 2; a base node out of range or not strictly ascending; a sign that is not +-1 or a first
 * sign of -1; a non-finite rhs; a negative or non-finite min_violation; a negative knob.  A non-finite entry of the cone's
 * part of primal: a host primal is checked by a host loop, a device primal by the reduction the triangle entry uses; the
 * message names the cone. */
typedef struct proxsdp_clique_cuts {
    int64_t struct_size;      /* = sizeof(proxsdp_clique_cuts) */
    int32_t on_device;        /* where primal lives: 0 host, 1 DEVICE pointer on the model's device (proxsdp_host_clique_cuts
                               * ignores it) */
    int32_t cone;             /* PSD cone of the model, 0-based in cone order (proxsdp_host_clique_cuts ignores it) */
    int32_t base_size;        /* q: 3 or 5 */
    int32_t grid, batch;      /* test knobs, 0 = default */
    int32_t reserved;
    int64_t n_base;           /* 1 .. 65536 */
    double  rhs;
    double  min_violation;    /* >= 0 */
    const double*  primal;    /* n doubles (proxsdp_host_clique_cuts ignores it: it is given X) */
    const int64_t* base_nodes;/* HOST, n_base x q */
    const int8_t*  base_sign; /* HOST, n_base x q */
    /* out: caller-allocated HOST arrays for n_base rows; k = q + 2 */
    int64_t* nodes;           /* k per row, ascending */
    int8_t*  signs;           /* k per row, the first +1 */
    double*  violation;
    int64_t* from_base;
    int64_t* add_col;         /* k (k - 1) / 2 per row */
    double*  add_val;         /* k (k - 1) / 2 per row */
    double*  add_h;
    int64_t n_rows;
    int64_t violated_bases;   /* bases whose best extension has v > min_violation, before merging */
    int64_t scanned;          /* n_base 4 C(s - q, 2) */
    int64_t bytes_allocated;  /* device bytes this call allocated (and released); 0 on the host */
    double  seconds;          /* wall time of the call */
    double  sweep_seconds;    /* the sweep kernels alone, between device events (0 on the host) */
} proxsdp_clique_cuts;
int  proxsdp_hip_model_cliques(proxsdp_model* mdl, proxsdp_clique_cuts* q);
/* The same contract with no device and no handle: a serial loop over the bases, the pairs in ascending order and the four
 * codes, keeping the first maximum.  X, cone_idx, index_base: as in proxsdp_host_triangle_cuts (only i < j of X is read).
 * PROXSDP_E_INVALID: as above where it applies; NULL X; side < q + 2 or > 46340; index_base other than 0 or 1; a non-finite
 * X_ij, i < j. */
int  proxsdp_host_clique_cuts(const double* X, int64_t side, const int64_t* cone_idx, int32_t index_base,
                              proxsdp_clique_cuts* q);
/* ------------------------------------------- rounding on a model handle: a +-1 vector from a PSD cone's factors
 * The verbs above tighten the relaxation's bound; this one produces a feasible point of a +-1 model (Max-Cut and its kin):
 * randomised hyperplane rounding (Goemans-Williamson) of the factors a solve hands out (proxsdp_psd_factors) to `trials`
 * sign vectors at once, each improved by a one-flip local search against the objective the handle holds NOW, and the best
 * one returned with its value.  The reference has no counterpart.  Everything below is fp64, evaluated left to right exactly
 * as written, with no contraction, on the device and on the host: the result is a pure function of the inputs, the same bits
 * on every run, whatever the launch and whatever the knobs.
 * IN.   cone: a PSD cone of the handle, side s >= 2.  V: s x r, column-major, ld = s; values: r numbers, finite and > 0 (the
 *       units of proxsdp_psd_factors; 1 <= r <= s).  on_device says where V and values live (device pointers are borrowed
 *       and trusted as proxsdp_model_data's are).  trials: T, a multiple of 64, 64 <= T <= 65536.  max_sweeps: 0 .. 1000,
 *       0 = rounding only.
 * WEIGHTS.     w_k = sqrt(values[k]), by std::sqrt on the HOST (device values cost one download of r doubles); no square
 *              root and no transcendental function runs on the device.
 * DIRECTIONS.  g(k, t) = (((u_0 + u_1) + ... + u_11) - 6.0), u_q = uniform53(seed, (t r + k) 12 + q): the counter-based
 *              generator of proxsdp_host_start_vector (integer operations, an exact conversion, twelve additions in order).
 * EMBEDDING.   y(i, t) = 0.0; for k = 0 .. r-1: y = y + (V[i, k] * w_k) * g(k, t).
 * SIGNS.       sigma_i = -1 if y < 0, else +1 (a zero row of V gives +1).
 * OBJECTIVE.   From the handle's CURRENT c in the caller's units (create's, or the last proxsdp_hip_model_update's), the
 *              cone's entries only: with var(i, j) the cone's variable of X_ij, d_i = c[var(i, i)], w_ij = c[var(i, j)] for
 *              i != j, adj(i) = the j != i with w_ij != 0, ascending.  The value of a sign vector is the cone's part of c'x
 *              at x = the triangle of sigma sigma':
 *                  f = 0.0;  for i ascending: f = f + d_i;
 *                  for i ascending: u = 0.0; for j in adj(i), j > i, ascending: u = u + w_ij * sigma_j;  f = f + sigma_i * u
 * SEARCH.      The library minimises (c is already sign-flipped for a MAX model).  A sweep visits i = 0 .. s-1: a = 0.0;
 *              for j in adj(i) ascending: a = a + w_ij * sigma_j with the signs as they are now; if sigma_i * a > 0, sigma_i
 *              is flipped at once.  Sweeps repeat until one flips nothing or max_sweeps have run.  The value after the
 *              search is computed afresh by the expression above, not accumulated from the flips.
 * ANSWER.      The trial with the smallest final value; among equal values the lowest t.
 * OUT (HOST arrays, caller-allocated): signs (s entries, +-1), best_trial, value, value_rounded (the smallest value BEFORE
 *       the search), sweeps (the most any trial ran, counting the sweep that flipped nothing), flips (the total over all
 *       trials); optional, NULL when not wanted: values_rounded[T], values_final[T], and the adjacency the library derived
 *       from c: adj_ptr[s + 1], adj_col / adj_val with room for adj_cap entries (adj_nnz written), diag[s] -- asked for by
 *       a non-NULL adj_ptr, which needs the other three.
 * The handle's data is not touched: a solve after the call equals a solve before it.  Scratch (the adjacency, 8 r T bytes
 * of directions, two copies of 8 s T / 64 bytes of sign words, 16 T bytes of values) is allocated in the call, released
 * before it returns and reported in bytes_allocated, not in proxsdp_model_info.device_bytes.
 * Other variables of the model are ignored, and the rows of A and G are NOT checked: any +-1 vector satisfies diag(X) = 1
 * and every triangle inequality at X = sigma sigma'; any other row is the caller's constraint to test.
 * How: the adjacency is built from the exit path's unscaled c on the device (count, prefix sum, ballot-compacted fill: the
 * values do not visit the host); k_round_directions writes g; k_round_signs has lane = trial and one ballot of y < 0 per node
 * and 64 trials gives a 64-bit word, words[i][T / 64]; k_round_search has one wave own 64 trials, walks the nodes in order
 * with the adjacency wave-uniform, each lane reading its bit, and XORs the ballot of sigma_i a > 0 into the node's word.  The
 * wave's word column lives in LDS for s <= lds_side (default 4096: 32 KiB), in global memory beyond.
 * Test knobs (0 = the library's choice; the result does not depend on any): grid_adjacency, grid_directions, grid_signs,
 * grid_search = workgroups of each launch; lds_side = the largest side whose words are kept in LDS (< 0: none, at most 8192).
 * PROXSDP_E_INVALID, decided on the host before any device call: a NULL struct or handle; a NULL V, values or signs; a wrong
 * struct_size; on_device other than 0 or 1; a cone number outside the model; a cone of side < 2; r outside 1 .. s; trials
 * not a multiple of 64 or outside 64 .. 65536; max_sweeps outside 0 .. 1000; a negative knob other than lds_side; an
 * adjacency asked for with a NULL adj_col / adj_val / diag or adj_cap smaller than its entries; a host `values` entry that is
 * not finite or not > 0; a non-finite host V.  Device factors are checked before anything else runs (V by a reduction,
 * values on their way to the weights); the message names the array. */
typedef struct proxsdp_rounding {
    int64_t struct_size;      /* = sizeof(proxsdp_rounding) */
    int32_t on_device;        /* where V and values live: 0 host, 1 DEVICE pointers on the model's device (proxsdp_host_round
                               * ignores it) */
    int32_t cone;             /* PSD cone of the model, 0-based in cone order (proxsdp_host_round ignores it) */
    int32_t r;                /* columns of V */
    int32_t trials;           /* T */
    int64_t seed;
    int32_t max_sweeps;
    int32_t grid_adjacency, grid_directions, grid_signs, grid_search, lds_side;   /* test knobs, 0 = default */
    const double* V;          /* s x r, column-major, ld = s */
    const double* values;     /* r */
    /* out: caller-allocated HOST arrays */
    int8_t*  signs;           /* s */
    double*  values_rounded;  /* T, or NULL */
    double*  values_final;    /* T, or NULL */
    int64_t* adj_ptr;         /* s + 1, or NULL = the adjacency is not wanted (proxsdp_host_round ignores these five) */
    int64_t* adj_col;         /* adj_cap */
    double*  adj_val;         /* adj_cap */
    double*  diag;            /* s */
    int64_t adj_cap;
    int64_t adj_nnz;          /* out (written when the adjacency is asked for) */
    int64_t best_trial;
    double  value, value_rounded;
    int64_t flips;
    int32_t sweeps;
    int32_t reserved;
    int64_t bytes_allocated;  /* device bytes this call allocated (and released); 0 on the host */
    double  seconds;          /* wall time of the call */
    double  search_seconds;   /* the search kernel alone, between two device events (0 on the host) */
} proxsdp_rounding;
int  proxsdp_hip_model_round(proxsdp_model* mdl, proxsdp_rounding* q);
/* The same contract with no device and no handle: a serial loop over the trials.  The adjacency is an argument: adj_ptr
 * (side + 1), adj_col / adj_val (adj_ptr[side] entries; per node ascending, none equal to the node, values finite; symmetry is
 * the caller's to keep) and diag (side).  PROXSDP_E_INVALID: as above where it applies; side < 2 or > 46340; a NULL or
 * malformed adjacency. */
int  proxsdp_host_round(int64_t side, const int64_t* adj_ptr, const int64_t* adj_col, const double* adj_val,
                        const double* diag, proxsdp_rounding* q);
/* g (r x trials doubles, row k contiguous) = the directions above.  PROXSDP_E_INVALID: NULL g, r < 1 or > 46340, trials as
 * above. */
int  proxsdp_host_round_directions(int64_t seed, int32_t r, int32_t trials, double* g);
/* ------------------------------------------- a certified dual bound of a model handle: a device Cholesky test
 * objval and dual_objval of a solve are estimates: the dual point is infeasible by dual_feasibility, and the lambda_min behind
 * that figure is a Lanczos Ritz value, which lies ABOVE the true eigenvalue -- the unsafe side.  This call returns a number
 * that IS a lower bound of the handle's optimum, whatever the dual point handed in.  It rests on no Lanczos run, no iterative
 * eigenvalue estimate and no tolerance of the solver: the proof is a COMPLETED floating-point Cholesky factorisation together
 * with its backward-error bound.  The reference has no counterpart.
 * THE BOUND.  The problem is min c'x, A x = b, G x <= h, x in its cones.  For any y_eq, any y_in and y_in+ = max(y_in, 0), with
 *       T_k >= tr X_k for every feasible x and Z_k = smat of cone k's part of c + A'y_eq + G'y_in+ (off-diagonals halved),
 *           c'x  >=  -b'y_eq - h'y_in+ + sum_k T_k min(0, lambda_min(Z_k))        for every feasible x,
 *       for a feasible y and for an infeasible one.  The call evaluates this with every rounding error pushed to the safe side.
 * SERVED.  Models whose variables all lie in PSD cones (side >= 1).  PROXSDP_E_UNSUPP, the message naming the reason: a
 *       second-order cone; a variable outside every cone; an equilibrated model.  (A handle never holds M_dense.)
 * IN.   dual_eq (p) and dual_in (m): both host or both device (on_device; device pointers are borrowed and trusted as
 *       proxsdp_model_data's are), in the units of a result.  trace_cap: HOST, one double per PSD cone (T_k), or NULL: T_k is
 *       then derived on the host from the model's CURRENT rows (create's, or the last proxsdp_hip_model_rows'): every diagonal
 *       variable of the cone must be the only stored entry of some equality row a X_ii = b with a != 0 and b / a >= 0; its cap
 *       is the smallest nextafter(b / a, +inf) over such rows, T_k the sum of the caps in order, each partial sum followed by
 *       nextafter(., +inf).  A cone with an uncovered diagonal returns PROXSDP_E_INVALID and names the cone.
 * 1. DUAL MATRIX AND RADIUS.  k_bound_dual_cone, one thread per column k of the model's unscaled [A; G] (cnt_k entries),
 *       contraction off: acc = 0; acc += val_q y_row(q) over the column in storage order; dc[k] = c[k] + acc -- the bits
 *       k_exit_dual_cone forms, with y_in+ in place of y_in -- and rad[k] = gamma(cnt_k + 2) (|c[k]| + sum |val_q| |y_row(q)|);
 *       both halved where k is an off-diagonal entry.  gamma(j) = j u / (1 - j u), u = 2^-53.  rho_k = the largest row sum of
 *       rad over the cone's matrix, every addition rounded up: it bounds ||Z_exact - Z~||_2.
 * 2. DUAL OBJECTIVE.  d = -sum_r bh_r y_r and D = sum_r |bh_r y_r| in one fixed-order reduction; d_safe = d - gamma(Q + 2) D.
 * 3. CERTIFIED lambda_min, per cone of side s >= 2 (side 1: l = dc - rad, rounded down).  Z~ is gathered into a dense s x s
 *       array (as k_tri_gather maps a cone's packed entries); nu = its largest absolute row sum.  For a shift sigma >= 0,
 *       A(sigma) = Z~ with fl(z_ii + sigma) on the diagonal.  The factorisation of A(sigma) either COMPLETES with every pivot
 *       above 2^-500 nu or reports its first failing column in a device flag; a non-positive or NaN pivot is a result, never
 *       an assert, a trap or a fault.  If it completes,
 *           lambda_min(Z~) >= -(sigma + delta),   delta = gamma(s + 3) / (1 - gamma(s + 3)) tr+(A) + u max_i |a_ii|,
 *       tr+ the diagonal sum rounded up.  First term: for a completed Cholesky factorisation in floating point
 *       |R~'R~ - A|_ij <= gamma(s + 1) (1 - gamma(s + 1))^-1 sqrt(a_ii a_jj) (Higham, Accuracy and Stability of Numerical
 *       Algorithms, 2nd ed., section 10.1, Theorem 10.3 and (10.7); Rump, Verification of positive definiteness, BIT 46 (2006));
 *       the matrix of the right-hand sides has rank one and 2-norm tr A, and R~'R~ is positive semidefinite.  The theorem holds
 *       for every order of summation and with fused multiply-adds, which is why the device may use MFMA and need not match
 *       the host's bits.  Second term: the rounding of the shifted diagonal.  The constant is not to be loosened.
 *       Shift search, decided only by completed / failed: sigma = 0; then sigma_j = nu 2^(-48 + 4 j), j = 0 .. 12, until one
 *       completes; when that was at j >= 1, five bisection steps between the last failure and the first success, each at the
 *       geometric mean (sqrt on the host); sigma* = the smallest completed shift.  At most 19 factorisations.  If sigma_12
 *       fails, certified[k] = 0, the cone's lambda_lower and the bound are -inf, and the call still returns 0.  (nu is
 *       rounded up, so sigma_12 >= ||Z~||_inf leaves positive pivots in exact arithmetic; what is not certified in practice
 *       is a cone whose nu or rho overflows: no factorisation is tried then, factorisations[k] = 0.)
 *       l_k = -(sigma* + delta(sigma*) + rho_k), the sums rounded up.
 * 4. COMBINATION, on the host: bound = d_safe + sum_k T_k min(0, l_k), every product and sum followed by nextafter(., -inf).
 * OUT.  bound, dual_objective (= d); per cone (HOST arrays, caller-allocated, n_psd entries): shift, lambda_lower, radius,
 *       factorisations, certified, and -- optional, NULL when not wanted -- delta and trace_used (T_k); bytes_allocated,
 *       seconds, factor_seconds (the factorisations with their flag read-backs).
 * The handle's data is not touched: a solve after the call equals a solve before it bit for bit.  Scratch (y, dc, rad, two
 * dense s x s arrays, row sums, the flag) is allocated in the call, released before it returns and reported in
 * bytes_allocated only.
 * How (csrc/dual_bound.hip.hpp): a right-looking blocked factorisation of the lower triangle with panels of 64 --
 * k_chol_diag (one workgroup, the 64 x 64 diagonal block in LDS, IEEE sqrt and division, sets the flag at a bad pivot),
 * k_chol_panel (the triangular solve of 64 rows per workgroup against the block in LDS), k_chol_update (A22 -= L21 L21' on
 * the lower-triangle tiles by v_mfma_f64_16x16x4_f64) -- chained as plain dependent launches on the model's stream: no waits
 * between workgroups, no atomics on doubles, every launch behind a set flag returns at once.  Each entry's accumulation order
 * is fixed by the code: the same input gives the same factor and the same flag on every run.  Sides that are no multiple of
 * 64 are handled by bounds in the kernels; the matrix is not padded.
 * PROXSDP_E_INVALID, on the host: a NULL struct, handle or array that is needed; a wrong struct_size; on_device other than 0
 * or 1; a non-finite host dual; a negative or non-finite cap.  Device duals are checked by a reduction on the device. */
typedef struct proxsdp_dual_bound {
    int64_t struct_size;      /* = sizeof(proxsdp_dual_bound) */
    int32_t on_device;        /* where dual_eq and dual_in live: 0 host, 1 DEVICE pointers on the model's device
                               * (proxsdp_host_dual_bound: must be 0) */
    int32_t reserved;
    const double* dual_eq;    /* p */
    const double* dual_in;    /* m */
    const double* trace_cap;  /* HOST, n_psd, or NULL = derive from the rows */
    /* out: caller-allocated HOST arrays, n_psd entries each */
    double*  shift;           /* sigma* (0 for side 1; +inf when not certified) */
    double*  lambda_lower;    /* l_k */
    double*  radius;          /* rho_k */
    int32_t* factorisations;
    int32_t* certified;
    double*  delta;           /* optional: delta(sigma*) */
    double*  trace_used;      /* optional: T_k */
    double  bound;
    double  dual_objective;   /* d */
    int64_t bytes_allocated;  /* device bytes this call allocated (and released); 0 on the host */
    double  seconds;          /* wall time of the call */
    double  factor_seconds;
} proxsdp_dual_bound;
int  proxsdp_hip_model_bound(proxsdp_model* mdl, proxsdp_dual_bound* q);
/* The same contract with no device and no handle: serial loops and the plain serial column Cholesky (column j: a_ij -= l_ik l_jk
 * for k < j in order, then the pivot test, sqrt and division).  c (n), M = [A; G] ((p + m) x n, CSC with base index_base, the
 * caller's variable order), bh = [b; h], and the PSD cone lists as proxsdp_problem holds them.  Sums run over a column in
 * storage order, so dc equals the device's wherever the stored order agrees; d may differ from the device's in its last bits
 * (another order), which D covers.  PROXSDP_E_INVALID: as above where it applies; a malformed matrix or cone list.
 * PROXSDP_E_UNSUPP: a variable outside every cone. */
int  proxsdp_host_dual_bound(int64_t n, int64_t p, int64_t m, const double* c, const proxsdp_csc* M, const double* bh,
                             int64_t n_psd, const int64_t* psd_ptr, const int64_t* psd_idx, int32_t index_base,
                             proxsdp_dual_bound* q);
/* test entries: ONE factorisation of A + shift I, with no model.  A: s x s HOST doubles, symmetric (the entries A[j * s + i],
 * i >= j, are read); 1 <= s <= 46340; the pivot floor is 2^-500 times the largest absolute row sum of A.  R_out (s x s,
 * row-major, may be NULL): the upper-triangular factor R = L' with zeros below the diagonal, R'R ~ A + shift I (after a failure
 * in the last panel of 64 columns the rows of R before fail_col hold the factor; otherwise only the rows of completed panels
 * do, the rest is unspecified).  fail_col: -1 = completed, else the first failing column, 0-based.
 * proxsdp_hip_cholesky runs the device kernels above; proxsdp_host_cholesky the plain serial column Cholesky of the host half. */
int  proxsdp_hip_cholesky(const double* A, int64_t s, double shift, double* R_out, int64_t* fail_col);
int  proxsdp_host_cholesky(const double* A, int64_t s, double shift, double* R_out, int64_t* fail_col);
/* test entry: the model's current internal data, downloaded into caller-allocated host arrays.  The sizes (n, Q = p + m, nnz,
 * ns = length of the support list, 0 when the support path is off) and the four norms (||b||, ||h||, ||c||, ||M||_F) are always
 * written; an array is written when its pointer is not NULL (call once with every pointer NULL for the sizes, allocate, call
 * again). */
typedef struct proxsdp_model_dump {
    int64_t struct_size;     /* = sizeof(proxsdp_model_dump) */
    int64_t n, Q, nnz, ns;                          /* out */
    double* csc_val; double* csr_val;               /* nnz each: the loop's scaled values, CSC / CSR */
    double* csc_val_orig; double* csr_val_orig;     /* nnz each: the exit path's unscaled values */
    double* c; double* c_orig;                      /* n each: c in solver order and scale; in solver order, unscaled */
    double* bh;                                     /* Q: [b; h] */
    int32_t* support; double* cS;                   /* ns each: the support list, c on it */
    double norms[4];                                /* out */
} proxsdp_model_dump;
int  proxsdp_hip_model_dump(proxsdp_model* mdl, proxsdp_model_dump* out);
/* test entry: ||v||_2 of n host doubles by the device route's reduction (k_model_norm2) with `grid` workgroups (<= 0: the
 * width an update uses).  The result does not depend on grid. */
int  proxsdp_hip_model_norm2(const double* v, int64_t n, int32_t grid, double* out);

/* test entry: the device exit path alone (Solver::cache_solution_device's launches) on host data.  x (n) is an internal iterate
 * in the solver's order and scale as the loop leaves it, y (p + m) the internal dual; zero_c != 0 takes c = 0 (the certificate
 * snapshot).  Out, on the host: the six vectors in the caller's order (any may be NULL); viol[4] = the violations of the
 * inequality duals, of the 1x1 cones, of the second-order cones and of the free variables; neg = minus the dual-cone block of
 * every PSD cone of side >= 2, one after the other in cone order, as the lambda_min run reads it (neg_cap doubles of room;
 * PROXSDP_E_INVALID when that is too little). */
int  proxsdp_hip_exit_vectors(const proxsdp_problem* prob, const proxsdp_options* opt, const double* x, const double* y,
                              int32_t zero_c, double* primal, double* dual_cone, double* dual_eq, double* dual_in,
                              double* slack_eq, double* slack_in, double* viol, double* neg, int64_t neg_cap);

/* ------------------------------------------- RCCL communicator helpers (block-sharded solves)
 * The library loads librccl at run time (dlopen; it does not link it).  One rank calls _unique_id and
 * ships the 128 bytes to the others by any means (MPI, torch.distributed, a file); every rank then calls
 * _comm_init on the GPU it owns and passes the handle as proxsdp_problem.nccl_comm.  A caller that already
 * has an ncclComm_t (created through the same librccl) passes it directly instead. */
int  proxsdp_hip_rccl_available(void);                      /* 1 = librccl loaded and usable */
int  proxsdp_hip_rccl_unique_id(void* id128);               /* NCCL_UNIQUE_ID_BYTES = 128 */
int  proxsdp_hip_rccl_comm_init(int32_t nranks, const void* id128, int32_t rank, int32_t device_id, void** comm);
int  proxsdp_hip_rccl_comm_destroy(void* comm);

/* ------------------------------------------- kernel-level test entry points
 * (not part of the drop-in; each is pinned against the oracle in tests/).
 * All pointers are host pointers; data is copied to the device, the kernel(s)
 * run, results are copied back. */

/* psd_projection! of ONE block given in packed svec form
 * (prox_operators.jl:33-66 with psd_vec_to_square/psd_square_to_vec :1-31).
 * mode 0: Lanczos path (krylovkit_eig!, :89-109) with nev = target_rank,
 *         falling back to full_eig! when not converged;
 * mode 1: full_eig! (:111-126) through the dense eigensolver;
 * mode 2: full_eig! served by the Lanczos engine (every positive eigenpair), target_rank = estimate
 *         of the number of positive eigenvalues; *out_fell_back = 1 if the dense solver had to run;
 * mode 3: full_eig! by the batched small-block Jacobi kernel (2 <= n <= 64); *out_converged = #{lambda > 0}.
 * mode 5: full_eig! by the one-workgroup, LDS-resident sign projection of small blocks (csrc/small_sign.hip.hpp; 2 <= n <= 64);
 *         *out_converged = #{lambda > 0} as in mode 3.
 * mode 4: full_eig! by the sign-function projection (options.full_eig_sign = 1): fp64 MFMA products, no eigenpairs;
 *         *out_rank = #{lambda > 0};
 * resid: start vector (n) or NULL.  out_*: rank (current_rank), min_eig,
 * nmatvec, converged eigenpairs, fell_back flag. */
int proxsdp_hip_psd_project(const double* packed_in, int64_t n, int32_t target_rank,
                            int32_t mode, const proxsdp_options* opt, const double* resid,
                            double* packed_out, int32_t* out_rank, double* out_min_eig,
                            int64_t* out_nmatvec, int32_t* out_converged, int32_t* out_fell_back);

/* Lanczos partial eigendecomposition of smat(packed) (eigsolver.jl:798-823):
 * vals (capacity cap), vecs (n x cap column-major); returns count in *out_count,
 * info.converged in *out_converged. */
int proxsdp_hip_eigsolve(const double* packed, int64_t n, int32_t nev,
                         const proxsdp_options* opt, const double* resid, int32_t cap,
                         double* vals, double* vecs, int32_t* out_count,
                         int32_t* out_converged, int64_t* out_nmatvec, int32_t* out_numiter);

/* y = smat(packed) * v, the Lanczos operator (dsymv('U') in the reference,
 * eigsolver.jl:678); repeat>1 re-launches for timing, *ms = mean kernel time. */
int proxsdp_hip_symv_packed(const double* packed, int64_t n, const double* v, double* y,
                            int32_t repeat, double* ms);

/* packed_out = svec(sum_k lambda_k z_k z_k') over lambda_k > 0
 * (fill! + rank-1 dgemm loop, prox_operators.jl:92-106, then :17-31) */
int proxsdp_hip_reconstruct(const double* Z, const double* lambda, int64_t n, int32_t r,
                            double* packed_out, int32_t repeat, double* ms);
/* the same with the kernel chosen explicitly: mfma = 0 scalar-FMA kernel (LDS-staged), 1 = fp64 MFMA
 * SYRK (v_mfma_f64_16x16x4_f64), -1 = the library's choice (options.reconstruct_mfma auto) */
int proxsdp_hip_reconstruct_kernel(const double* Z, const double* lambda, int64_t n, int32_t r, int32_t mfma,
                                   double* packed_out, int32_t repeat, double* ms);

/* *resid2 = ||X - V diag(lam) V'||_F^2 and *xnorm2 = ||X||_F^2 for X = smat(packed) with PLAIN entries (upper triangle
 * column by column, no sqrt(2)) of side n, V n x r column-major with leading dimension ldv >= n (rows n .. ldv-1 are never
 * read), both norms over the full symmetric matrix: k_factor_residual, the MFMA SYRK tiling of the reconstruction with the
 * tiles' partial sums added in tile order.  r = 0 (V, lam may be NULL): *resid2 = *xnorm2. */
int proxsdp_hip_factor_residual(const double* packed, int64_t n, const double* V, int64_t ldv,
                                const double* lam, int32_t r, double* resid2, double* xnorm2);
/* the same, timed: repeat > 0 re-launches the kernel on the device-resident data, *ms = mean kernel time (events); the sums
 * returned are then those of one more launch after the timed ones (the kernel only reads the block: they are the same) */
int proxsdp_hip_factor_residual_kernel(const double* packed, int64_t n, const double* V, int64_t ldv,
                                       const double* lam, int32_t r, double* resid2, double* xnorm2,
                                       int32_t repeat, double* ms);

/* full_eig! (prox_operators.jl:111-126) of one packed block, timed: sign = 0 rocSOLVER dsyevd + reconstruction,
 * 1 = the sign-function projection (options.full_eig_sign) with the default options.sign_start_row, 100 + k = the
 * same with sign_start_row = k (100: the full table); ms = wall time per call over `repeat` calls on
 * device-resident data, out_rank = #{lambda > tol_psd} (dsyevd) / #{lambda > 0} (sign), out_products = MFMA
 * products per call (averaged over the warm-up call and the timed ones) */
int proxsdp_hip_full_eig_kernel(const double* packed_in, int64_t n, int32_t sign, double* packed_out,
                                int32_t repeat, double* ms, int32_t* out_rank, int64_t* out_products);

/* Mx = M x (pdhg.jl:634) and Mty = M' y (pdhg.jl:556) for M given as CSC */
int proxsdp_hip_spmv(const proxsdp_csc* M, int32_t index_base, int32_t transpose,
                     const double* in, double* out);

/* x_out = x - tau (Mty + c)   (primal_step!, pdhg.jl:622; fused AXPY kernel, FP contraction off) */
int proxsdp_hip_primal_update(const double* x, const double* Mty, const double* c, double tau, int64_t n,
                              double* x_out);

/* one linesearch trial in y-space (pdhg.jl:547-553 + box_projection!, prox_operators.jl:160-170):
 *   ybar = y + bt ((1+theta) Mx - theta Mx_old);  y_out = ybar - bt * box(ybar / bt)
 * with box = b on the first p rows and min(., h) on the rest (bh = [b;h]);
 * ynorm2 = |y_out - y|^2 (the right-hand side of the acceptance test, :566) */
int proxsdp_hip_dual_trial(const double* y, const double* Mx, const double* Mx_old, const double* bh,
                           int64_t p, int64_t Q, double bt, double theta, double* y_out, double* ynorm2);

/* compute_residual! + compute_gap! (residuals.jl:2-71), the reductions only.  out[9]:
 *   0 max|(x - tau Mty) - (x_old - tau Mty_old)|   1 max|x_old - tau Mty_old|   2 c'x
 *   3 max|(y - sigma Mx) - (y_old - sigma Mx_old)| 4 max|y_old - sigma Mx_old|
 *   5 max|Mx - b| (equalities)  6 max(0, max(Mx - h)) (inequalities)  7 b'y_eq  8 h'y_in */
int proxsdp_hip_residuals(const double* x, const double* x_old, const double* Mty, const double* Mty_old,
                          const double* c, double tau, int64_t n,
                          const double* y, const double* y_old, const double* Mx, const double* Mx_old,
                          const double* bh, int64_t p, int64_t Q, double sigma, double* out);

/* ONE batch of linesearch candidates (linesearch! / dual_step!, pdhg.jl:532-609, with the reductions of compute_residual! /
 * compute_gap!, residuals.jl:2-71) through the solver's own launches, on host data.  M = [A;G] (Q x n, CSC in storage order),
 * rows 0 .. p-1 equalities.  Candidate k takes tau[k], theta[k], bt[k], sigma[k]:
 *   y+_k = ybar - bt box(ybar / bt), ybar = y + bt ((1 + theta) Mx - theta Mx_old);  plain = 0: stored as (y+ - y) + y and
 *   (M'y+ - Mty_old) + Mty_old (linesearch!'s in-place norm and revert), plain = 1: as computed (dual_step!).
 * x is the new iterate, x_old the previous one (weighted by xold_coef in the residual), Mx = M x, Mx_old = M x_old.
 * support = 1: the support-aware path, S = {i : column i non-empty or c_i != 0}; M'y+ is computed on S only, and
 * k_primal_update_S runs first on x_old with step tau_update and M'y = Mty_old (x_upd, xsave, esv).
 * scal: 11 per candidate -- 0 |y+ - y|^2 (rows weighted by roww)  1 |M'y+ - Mty_old|^2  2..4 and 5..10 as out[0..2] and
 * out[3..8] of proxsdp_hip_residuals (b'y, h'y weighted by roww on the support path).
 * support = 2: the general path as a shard of a block-sharded solve runs it -- as support = 0, but b'y and h'y (slots 9, 10)
 * are weighted by roww too; with support = 0 they stay unweighted whatever roww is.
 * c0 >= 0: afterwards candidate c0's residuals (slots 2..10) are evaluated again with tau_re / sigma_re into scal_re[11]. */
typedef struct {
    int64_t struct_size;
    /* in */
    int64_t p;
    const double* bh; const double* y; const double* Mx; const double* Mx_old;        /* Q each */
    const double* x; const double* x_old; const double* Mty_old;                      /* n each, as c (an argument of the call) */
    const double* roww;                  /* Q row weights of a block-sharded solve, or NULL */
    double xold_coef, tau_update;
    int32_t support, nc, plain, c0;      /* support = 0, 1 or 2 (above); nc = 1..3; c0 < 0: no re-evaluation */
    double tau[3], theta[3], bt[3], sigma[3];
    double tau_re, sigma_re;
    /* out */
    double* y_out;                       /* nc x Q */
    double* Mty_out;                     /* nc x ns, ns = |S| (support) or n; capacity nc x n */
    double* scal;                        /* nc x 11 */
    double* scal_re;                     /* 11 (c0 >= 0) */
    int32_t* supp_out;                   /* support = 1: S ascending, capacity n */
    double* x_upd; double* xsave; double* esv;   /* support = 1: n, capacity n, capacity 2 n ([2][ns]) */
    int64_t ns;
    int32_t gq, gx;                      /* workgroup columns of the y passes and of the x / column passes */
} proxsdp_trial_batch;
int proxsdp_hip_trial_batch(const proxsdp_csc* M, int32_t index_base, const double* c, proxsdp_trial_batch* t);

/* The non-PSD tail of the projection on host data (n entries): nsoc second-order cones at soc_off / soc_len (x[off] the
 * scalar part; soc_projection!, prox_operators.jl:145-158) and n_one 1x1 PSD blocks at one_off (:43-45).  x_soc = x after the
 * SOC projection, gap_in / gap_out = |v| - s per cone before / after it (residuals.jl:73-86), x_clamp = x_soc after
 * x = max(0, x) on the 1x1 blocks, min_eig their values. */
int proxsdp_hip_cone_tail(const double* x, int64_t n, const int64_t* soc_off, const int32_t* soc_len, int32_t nsoc,
                          const int64_t* one_off, int32_t n_one, double* x_soc, double* gap_in, double* gap_out,
                          double* x_clamp, double* min_eig);

/* ONE PSD projection of an n-vector through the solver's own phases, with no launch of its own: setup_device, classify_blocks
 * (with the blocks' workspaces), setup_small_batch, setup_soc, an upload of x, psd_projection(x) at iteration 1, a stream
 * synchronisation, harvest_small_ranks.  The problem is used for its cone layout only (PSD sides, 1x1 included, SOCs, free
 * variables; it may have no rows); x is in the solver's internal order and scaling (cone variables first, in cone order,
 * off-diagonal PSD entries times sqrt 2), as the vectors of proxsdp_state are.  The projection touches the PSD blocks only.
 * Per PSD block: offset and side; block_class = 0 a 1x1 block (clamped), 1 one-launch Jacobi (k_small_psd_project), 2 one-launch
 * sign function (k_small_sign_project), 3 large (an engine per block); rank = current_rank; min_eig (1x1 blocks: the clamped
 * value the kernel recorded); sweeps = Jacobi sweeps run (class 1; -1 elsewhere).  Non-finite values in a block come back as
 * PROXSDP_E_HIP with the message of the engine that met them. */
typedef struct {
    int64_t struct_size;
    /* in */
    const double* x;                     /* n */
    /* out */
    double* x_out;                       /* n */
    int64_t* block_off; int32_t* block_side; int32_t* block_class;    /* n_psd each */
    int64_t* rank; double* min_eig; int32_t* sweeps;                   /* n_psd each */
    int64_t batched_small_eigs, full_eigs, full_eigs_sign, sign_short_pass, sign_short_fail;    /* proxsdp_stats of the call */
} proxsdp_project_cones;
int proxsdp_hip_project_cones(const proxsdp_problem* prob, const proxsdp_options* opt, proxsdp_project_cones* t);

/* ONE product of the sign-function projection (full_eig! without an eigendecomposition, prox_operators.jl:111-126) through the
 * solver's own launch code (Solver::sym_gemm), on host data: k_sym_gemm (tile = 64), k_sym_gemm32 (32) or k_sym_gemm48 (48).
 * P, Q, Y: symmetric n x n, column-major; they are zero-padded to ld = 64 ceil(n / 64) as the solver's work matrices are.
 * With m_i = dsc[i] (use_dsc != 0) or 1:
 *   epilogue 0 (plain): T = m0 P Q                                   part: Frobenius^2 partials of T
 *   epilogue 1 (poly) : T = ca m0 I + cb m1 Y + cc m2 P Q            (the identity term on the WHOLE diagonal, padding included)
 *   epilogue 2 (final): packed xp = (P + m0 P Q) / 2, off-diagonals x sqrt(2)     part: partials of the trace of Q[:n, :n]
 *   epilogue 3        : as 2 with the fused residual partials: over the entries whose bit mask_off + index is CLEAR in mask,
 *                       respart[0][w] = max |xp - xold|, respart[1][w] = max |xold| of workgroup w's tile
 * The upper triangle of T holds the computed product, the lower one its mirror.  T (ld x ld), part, xp and respart are
 * prefilled with `sentinel`, so that the caller sees what the launch wrote.  part may be NULL for epilogues 0 and 1 (no
 * partials are formed then).  Refused with PROXSDP_E_INVALID: tile = 48 where the solver's rule refuses it (48 ceil(n / 48) > ld,
 * or the 72 KiB of dynamic LDS were not granted), tile = 32 or 48 with epilogue 2 or 3. */
typedef struct {
    int64_t struct_size;
    /* in */
    int32_t n, tile, epilogue, use_dsc;
    const double* P; const double* Q; const double* Y;   /* n x n each; Y: epilogue 1 only */
    double ca, cb, cc;
    double dsc[3];
    const double* xold;                  /* epilogue 3: packed, n (n + 1) / 2 */
    const uint32_t* mask; int64_t mask_words, mask_off;   /* epilogue 3: support bits; 32 mask_words >= mask_off + n (n + 1) / 2 */
    double sentinel;
    /* out */
    double* T;                           /* ld x ld (epilogues 0, 1) */
    double* part;                        /* one slot per launched workgroup; capacity >= (ld / 32 + 1)^2 / 2 + 8 */
    double* xp;                          /* n (n + 1) / 2 (epilogues 2, 3) */
    double* respart;                     /* 2 x grid (epilogue 3) */
    int32_t ld, grid;                    /* leading dimension of T, workgroups launched */
} proxsdp_sym_product;
int proxsdp_hip_sym_product(proxsdp_sym_product* t);

/* The head of a sign-function projection of one packed block of side n, as Solver::full_eig_by_sign launches it:
 * k_unpack_sym (A = smat(packed) in full storage; A, ld x ld, is prefilled with `sentinel`: the kernel writes the n x n leading
 * part only), k_sign_scalars stage 0, the first product Y0 = A A / f^2 on the tile shape the solver chooses (on a zero-padded
 * A), k_sign_scalars stage 1.  sc[16]: sc[0] = 1 / f^2, sc[6] = f = ||A||_F, sc[1] = 1 / s, sc[4] = s = f sqrt(g) with
 * g = ||Y0||_F, sc[8..10] = {1, 1 / g, 1 / g^2}; the other slots are zero. */
int proxsdp_hip_sign_unpack(const double* packed, int64_t n, double sentinel, double* A, double* sc);

/* ONE rank-r reconstruction of a packed block through the solver's own launch code (Solver::launch_reconstruct, called as
 * ritz_pairs_to_block calls it on the support path), on host data: k_reconstruct_packed<FUSE_RES> or k_reconstruct_mfma<FUSE_RES>,
 *   xp[(i, j)] = s_ij sum_k lam[k] Z[i, k] Z[j, k],  s = sqrt(2) off the diagonal, 1 on it   (prox_operators.jl:92-106, 17-31).
 * Z: ldz x r column-major, ldz >= n; the rows n .. ldz-1 are never read.  mfma = 0 / 1 forces the scalar / the MFMA kernel,
 * -1 leaves the choice to the solver (MFMA from r = 16 on).
 * xold != NULL: the fused launch of the support path.  The block is the one at packed offset mask_off of a vector whose support
 * bits are `mask` (bit mask_off + idx of entry idx), its residual slots are slots 0 .. grid-1 of a buffer of stride grid: over the
 * entries whose bit is CLEAR, respart[b] = max |xp - xold| and respart[grid + b] = max |xold| of workgroup b's tile; the padding
 * workgroups write nothing.  xold = NULL: the unfused launch with the same ldz; respart is never written.
 * xp (n (n + 1) / 2) and ALL respart_cap >= 2 grid entries of respart are prefilled with `sentinel`, so that the caller sees what
 * the launch wrote and that nothing was written behind 2 grid.  Refused with PROXSDP_E_INVALID: r < 0, ldz < n,
 * 32 mask_words < mask_off + n (n + 1) / 2, mask_off < 0, respart_cap < 2 grid (grid = 8 ceil(nt (nt + 1) / 16), nt = ceil(n / 64)). */
typedef struct {
    int64_t struct_size;
    /* in */
    int32_t n, r, ldz, mfma;
    const double* Z; const double* lam;          /* ldz x r, r (both may be NULL when r = 0) */
    const double* xold;                          /* packed, n (n + 1) / 2, or NULL: unfused */
    const uint32_t* mask; int64_t mask_words, mask_off;
    int64_t respart_cap;
    double sentinel;
    /* out */
    double* xp;                                  /* n (n + 1) / 2 */
    double* respart;                             /* respart_cap */
    int32_t grid, kernel;                        /* workgroups launched; 0: k_reconstruct_packed ran, 1: k_reconstruct_mfma */
} proxsdp_reconstruct_fused;
int proxsdp_hip_reconstruct_fused(proxsdp_reconstruct_fused* t);

/* ONE basis rotation out[:, c] = sum_j V[:, j] U[j, c], c < ncols (the restart rotation and the final Ritz vectors of the
 * Lanczos driver; KrylovKit basistransform!) through Solver::rotate -- the pinned staging copy of U, its upload, then
 * Solver::rotate_launch: k_lz_rotate (one or several launches), k_lz_rotate_mfma or k_lzw_rotate -- on a workspace sized as an
 * eigsolve sizes it for the Krylov dimension max(K, Kv - 1, out_cols - 1).  V: n x Kv column-major, Kv >= max(K, copy_src + 1);
 * it is zero-padded to npad = 64 ceil(n / 64) rows, as the step kernels keep the basis.  U: K x ncols, compact column-major.
 * Behind U, in the same upload, ride 8 NaN where a restart puts its arrow part: reading past row K of a column of U shows.
 * copy_src >= 0: out[:, copy_dst] = V[:, copy_src] as well (the residual column of a restart).  wide = 1: the rotation of a
 * wide run (Krylov dimension 256 .. 511, options.lanczos_wide_krylov), which needs the wide workspace.
 * out: npad x out_cols, prefilled with `sentinel`.  form: which kernel ran (PROXSDP_ROTATE_*, 0 when nothing was launched),
 * launches: how many launches it took.  Refused with PROXSDP_E_INVALID: ncols < 0 or > K, K < 1, Kv too small, copy_dst or
 * ncols outside out_cols, wide = 1 with a Krylov dimension <= 255 (no wide workspace), wide = 0 with one > 255. */
#define PROXSDP_ROTATE_SCALAR 1
#define PROXSDP_ROTATE_MFMA   2
#define PROXSDP_ROTATE_WIDE   3
typedef struct {
    int64_t struct_size;
    /* in */
    int32_t n, K, ncols, Kv, copy_src, copy_dst, wide, out_cols;
    const double* V; const double* U;
    double sentinel;
    /* out */
    double* out;                                 /* npad x out_cols */
    int32_t npad, form, launches, reserved;
} proxsdp_rotation;
int proxsdp_hip_rotate(proxsdp_rotation* t);

/* The support path's copy of the non-PSD tail (k_tail_copy_res through Solver::launch_tail_copy) on `wgs` workgroups:
 * xout[i] = xin[i] for start <= i < N (xout, N entries, is prefilled with `sentinel`), and per workgroup w
 * respart[w] = +0 (x_new = x_old there), respart[wgs + w] = max |xin[i]| over the entries i = start + 256 w + t (+ 256 wgs ..)
 * of its grid stride whose bit i of `mask` is CLEAR.  Refused with PROXSDP_E_INVALID: start < 0 or >= N, wgs < 1,
 * 32 mask_words < N. */
typedef struct {
    int64_t struct_size;
    /* in */
    int64_t N, start;
    const double* xin;
    const uint32_t* mask; int64_t mask_words;
    int32_t wgs, reserved;
    double sentinel;
    /* out */
    double* xout;                                /* N */
    double* respart;                             /* 2 x wgs */
} proxsdp_tail_copy;
int proxsdp_hip_tail_copy(proxsdp_tail_copy* t);

/* Every cycle of ONE thick-restart Lanczos run on a packed block, as the production driver Solver::lanczos leaves it: the
 * entry installs the driver's per-cycle observer (called between the read-back of a cycle's record and the restart logic, the
 * basis final and not yet rotated), sets the run's maxiter to max_cycles and calls Solver::lanczos -- the engine lz_plan
 * chooses, the split cycle with the host or device merge, the speculated first mat-vec and the one-workgroup kernel's deferred
 * rotation run as in a solve.  opt (NULL: the defaults) passes through: eigsolver_min_lanczos, lanczos_cycle_kernel,
 * lanczos_wide_krylov, host_eig_merge, device_eig_merge, eigsolver, krylovkit_tol, ...; krylovkit_max_iter / arpack_max_iter
 * are overwritten with max_cycles.  resid: the start vector (n entries, normalised by the library), NULL: the library's own.
 * krylovdim = max(2 nev + 1, eigsolver_min_lanczos); the caller states cols = krylovdim + 1 and ldv = 64 ceil(n / 64) and
 * allocates, per cycle c < max_cycles: info + PROXSDP_LZ_INFO c, V + c cols ldv, alphas / betas / D / f + c cols.  All are prefilled with the
 * sentinel (info: -1).  For each cycle the driver ran (`cycles` of them):
 *   info[0] kfirst (the kept columns; 0 in the first cycle), info[1] Kend (krylovdim, or kstop when the stop flag is set),
 *   info[2] the stop flag, info[3] the engine (PROXSDP_LZ_ENGINE_*), info[4] 1 when the cycle was a split cycle,
 *   info[5] 1 when its first mat-vec had been speculated by the cycle before, info[6] 1 when the preceding restart's merge ran
 *   on the device, info[7] 1 when the first phase of the split eigensolve succeeded for this cycle, info[8] 1 when the kept
 *   columns were compared with what the cycle was handed -- after a restart on the step or wide engine the entry repeats the
 *   restart rotation (Solver::rotate_launch on the previous basis and the coefficients still on the device) into a buffer of
 *   its own -- and info[9] the number of entries of the columns 0 .. kfirst, padding rows included, whose bits differ from it
 *   (the one-workgroup kernel rotates in its own prologue: info[8] = 0 there), info[10 .. 11] reserved;
 *   V: ALL cols columns of the basis buffer at stride ldv, padding rows included -- columns 0 .. Kend are the cycle's basis
 *   (column Kend is not written by a cycle that stopped), the columns behind hold what earlier cycles or the zeroed
 *   workspace left there; alphas[kfirst .. Kend), betas[kfirst .. Kend) from the cycle's record;
 *   D[0 .. kfirst), f[0 .. kfirst): the arrow part the cycle ran with (Ritz values and couplings of the kept columns).
 * Refused with PROXSDP_E_INVALID before a device is touched: nev < 1 or > n, max_cycles < 1, cols / ldv not as stated above,
 * krylovdim > 255 without opt->lanczos_wide_krylov = 1 or > 511 with it (beyond the workspace), krylovkit_eager (another driver). */
#define PROXSDP_LZ_ENGINE_STEP   0
#define PROXSDP_LZ_ENGINE_BLOCK1 1
#define PROXSDP_LZ_ENGINE_WIDE   2
#define PROXSDP_LZ_INFO          12
typedef struct {
    int64_t struct_size;
    /* in */
    int32_t n, nev, max_cycles, cols, ldv, reserved;
    const double* packed;                        /* n (n + 1) / 2 */
    const proxsdp_options* opt;
    const double* resid;                         /* n, or NULL */
    double sentinel;
    /* out */
    int32_t* info;                               /* max_cycles x PROXSDP_LZ_INFO */
    double* V;                                   /* max_cycles x cols x ldv */
    double* alphas; double* betas; double* D; double* f;   /* max_cycles x cols each */
    int32_t npad, krylovdim, cycles, reserved2;
} proxsdp_lanczos_cycles;
int proxsdp_hip_lanczos_cycles(proxsdp_lanczos_cycles* t);

/* Every cycle of ONE thick-restart Lanczos run on the OPERATOR FORM, A v = F (lam o (F' v)) + E v: as proxsdp_hip_lanczos_cycles
 * (the same observer, the same arrays per cycle, info[0 .. 9] as there), but the block of side n is given by its pieces and no
 * packed block exists.  support: ns strictly ascending packed indices (column-major upper triangle, k = i + j (j + 1) / 2,
 * i <= j) below n (n + 1) / 2; esv: the support-value array as the solver holds it, 2 ns values in svec units (an off-diagonal
 * entry carries the sqrt(2)): [0, ns) is what the kernels read beside factors, [ns, 2 ns) what they read in the second form.
 * F (n x rp, column-major) and lam (rp positive values), 0 <= rp <= 127, rp <= n: the previous projection's factors; they are
 * put into the factor buffer from column f_first on (0 <= f_first <= 127), as a dsaupd-rule projection leaves them.
 * no_factors = 1: the second form, x_prev has no factors (rp must be 0) and E takes the values esv + ns.  The ELL / overflow
 * layout is built by the solver's own set-up code from the support list; a row of more than 32 entries needs
 * opt->lanczos_operator = 1 below side 6000, as in a solve.  probe_v (n values, or NULL): before the run ONE mat-vec launch on
 * the records form with v = probe_v: probe_ev (ldv) = E v, probe_tpart (ceil(n / 64) x 128) the per-row-block records of F' v
 * (record g, column c at 128 g + c), probe_apart (ceil(n / 64)) the row blocks' shares of v' E v.
 * Per cycle, beside info[0 .. 9]: info[10] the mat-vecs the cycle ran on the operator-form kernels, info[11] 1 on the owner
 * form of F' v (0: the records form), info[12] the factor-column chunks of 64 the kernels were built for (1 or 2), info[13] the
 * ELL width, info[14] the rows with overflow entries, info[15] for the one-workgroup kernel 1 when E sat in LDS, 0 when it
 * was read through L2, -1 on the step kernels.  ell_w / overflow_rows: the same two numbers, known before the run.
 * Refused with PROXSDP_E_INVALID before any launch: n outside 2 .. 46340, nev outside 1 .. n, max_cycles < 1, cols / ldv not
 * krylovdim + 1 / 64 ceil(n / 64), a Krylov dimension above 255 (the operator form runs on the step kernels and the
 * one-workgroup kernel only), krylovkit_eager, lanczos_operator = 0, rp or f_first out of range, no_factors with rp > 0, an
 * index out of range or not ascending, a value of the active half of esv, of F, lam, resid or probe_v that is not finite,
 * lam <= 0, a NULL array. */
#define PROXSDP_OP_INFO          16
typedef struct {
    int64_t struct_size;
    /* in */
    int32_t n, nev, max_cycles, cols, ldv, rp;
    int32_t f_first, no_factors;
    int64_t ns;
    const int32_t* support;                      /* ns */
    const double* esv;                           /* 2 ns */
    const double* F;                             /* n x rp */
    const double* lam;                           /* rp */
    const proxsdp_options* opt;
    const double* resid;                         /* n, or NULL */
    const double* probe_v;                       /* n, or NULL */
    double sentinel;
    /* out */
    int32_t* info;                               /* max_cycles x PROXSDP_OP_INFO */
    double* V;                                   /* max_cycles x cols x ldv */
    double* alphas; double* betas; double* D; double* f;   /* max_cycles x cols each */
    double* probe_ev; double* probe_tpart; double* probe_apart;   /* with probe_v */
    int32_t npad, krylovdim, cycles, ell_w;
    int32_t overflow_rows, reserved;
} proxsdp_operator_cycles;
int proxsdp_hip_operator_cycles(proxsdp_operator_cycles* t);

/* ONE positive-part run of the Lanczos engine (full_eig! served by it: Solver::lanczos(W, xp, nev, true)) and its per-call
 * certificate (Solver::lanczos_certificate), as Solver::full_eig_by_lanczos runs them one after the other.  The block, the
 * options, the start vector and the per-cycle arrays are those of ONE of the two entries above: packed_run or operator_run, the
 * other NULL; the struct pointed to is validated, prefilled and filled per cycle exactly as by its own entry, with two
 * differences: the run is the positive-part run, and the workspace is sized for ws_rank pairs, cap = min(max(2 min(max(ws_rank,
 * 2), n) + 1, eigsolver_min_lanczos), 255) + 1 columns (lanczos_wide_krylov is read as 0).  The caller states cap, and in the
 * wrapped struct cols = krylovdim + 1 of the positive-part run: krylovdim = min(min(cap, 256) - 1, max(max(2 nev + 1,
 * eigsolver_min_lanczos), nev kdim10 / 10 + 8)), kdim10 = full_eig_lanczos_kdim10 (30 when not positive) -- a small ws_rank
 * gives the clipped dimension krylovdim = cap - 1.
 * run = 1: the run.  converged / count / numiter: what it returned; vals[0 .. count); Z: its Ritz vectors, count columns at
 * stride ldv, padding rows included; warm = 1 when lz_start_basis took the warm path (k_lz_warm_sum / k_lz_warm_scale).  vals
 * and Z hold `sentinel` (the wrapped struct's) where nothing was written.  run = 0: no run; the wrapped struct's per-cycle arrays
 * stay prefilled, cycles = 0, and the run's parameters and plan are set by lz_init / lz_plan alone.
 * cert_steps >= 2: then the certificate.  It locks the run's own result (npos_in = -1, needs run = 1; skipped with cert_ran = 0
 * when the run did not converge) or the caller's set: locked (n x npos_in, column-major, orthonormal), locked_vals (npos_in,
 * descending as a run leaves them), npos_in >= 0, put where lz_finish_run leaves a run's result (columns 0 .. npos_in of the
 * Ritz-vector buffer with zero padding rows, and the workspace's values).  Before the call the columns from npos on of that
 * buffer are filled with the sentinel, padding rows included, and the columns 0 .. npos and the values are kept aside.
 *   cert_ran: the function's return value (0 as well when npos + cert_steps + 1 > cap: nothing is written then);
 *   npos: the locked pairs; theta_max, scale: its results; posres: the factor of the caller's test theta_max <= posres scale
 *   (Solver::lanczos_posres); steps: the steps that formed the tridiagonal (after the cut at kstop), stop / kstop: the control
 *   block; cert_alphas / cert_betas (cap each): [npos .. npos + cert_steps) from the record, the sentinel elsewhere;
 *   basis (cap x ldv): the whole Ritz-vector buffer after the call; resid2 (ldv): the second start vector; differ: the number
 *   of doubles of the columns 0 .. npos, padding rows included, and of the values whose bits are no longer those kept aside;
 *   matvecs: the mat-vecs the certificate counted.
 * Refused with PROXSDP_E_INVALID before a device is touched and before an output array is written: whatever the wrapped entry
 * refuses but a Krylov-branch dimension max(2 nev + 1, eigsolver_min_lanczos) above 255 (the run's is clipped), both or neither of the two
 * pointers, cap or cols not as stated, ws_rank < 1, run / cert_steps / npos_in out of range, run = 0 without a locked set,
 * npos_in > n, a locked entry or value that is not finite, a NULL array. */
typedef struct {
    int64_t struct_size;
    /* in */
    proxsdp_lanczos_cycles* packed_run;          /* one of the two */
    proxsdp_operator_cycles* operator_run;
    int32_t ws_rank, cap, run, cert_steps;
    int32_t npos_in, reserved;
    const double* locked;                        /* n x npos_in */
    const double* locked_vals;                   /* npos_in */
    /* out: the run */
    int32_t converged, count, numiter, warm;
    double* vals;                                /* cap */
    double* Z;                                   /* cap x ldv */
    /* out: the certificate */
    int32_t cert_ran, npos, steps, stop;
    int32_t kstop, reserved2;
    int64_t differ, matvecs;
    double theta_max, scale, posres;
    double* cert_alphas; double* cert_betas;     /* cap each */
    double* basis;                               /* cap x ldv */
    double* resid2;                              /* ldv */
} proxsdp_positive_part;
int proxsdp_hip_positive_part(proxsdp_positive_part* t);

/* host only: the doubles of dynamic LDS the one-workgroup cycle kernel asks for (b1_lds_plan) at nt = ceil(n / 64) row blocks
 * -- fop = 0: the packed operator with a triangle of xN entries resident; fop = 1: the operator form with ell_w_lds ELL
 * columns of E resident (0: E read through L2).  -1: nt outside 1 .. 8, or a negative size. */
int64_t proxsdp_host_block1_lds_doubles(int32_t nt, int32_t fop, int64_t xN, int32_t ell_w_lds);

/* The "Init" section (pdhg.jl:54-142) of a solve with a dense A (prob->M_dense), nothing more: E (p + m) and D (n), the
 * equilibration diagonals -- ones when equilibration is off or switched itself off, *equilibrated says which --, frob =
 * ||.||_F and sigma_max = the largest singular value of the solver's matrix E [A;G] D S (S: the sqrt(2)/2 factor on
 * off-diagonal PSD columns).  sigma_max is computed only when opt->approx_norm = 0, otherwise it is 0.  Any output may
 * be NULL. */
int proxsdp_hip_dense_scaling(const proxsdp_problem* prob, const proxsdp_options* opt,
                              double* E, double* D, double* frob, double* sigma_max, int32_t* equilibrated);

/* The coupling-row sum of an in-process shard group (k_coupling_sum, through the solver's own launch code) on host data:
 * parts = n_shards partial buffers of `len` doubles each (row-major n_shards x len), rows = len row numbers into a vector of
 * n doubles (each in 0 .. n-1, otherwise PROXSDP_E_INVALID; they should be distinct).  v_out = v_in with
 * v_out[rows[k]] = ((parts[0][k] + parts[1][k]) + parts[2][k]) + ... */
int proxsdp_hip_coupling_sum(const double* parts, int32_t n_shards, int64_t len, const int64_t* rows,
                             const double* v_in, int64_t n, double* v_out);

/* ------------------------------------------- host-only helpers (no GPU needed;
 * exercised by the CPU test-suite) */
/* One shard of proxsdp_hip_solve_sharded's split (csrc/shard_split.hpp: the C++ restatement of sharded.py's
 * split_block_diagonal), all arguments as there.  The sizes are always written; an array is written when its pointer is not
 * NULL (call once with every pointer NULL for the sizes, allocate, call again).  Everything that comes out is 0-BASED,
 * whatever prob->index_base: vars / rows_eq / rows_in = the caller's variable and row numbers the shard holds (ascending),
 * coupling_rows = positions in the shard's own row numbering (equalities first), psd_ids / soc_ids = the caller's cone
 * numbers, psd_idx / soc_idx = the shard's own variable numbers, eig_resid = the shard's share of prob->eig_resid (the
 * vectors of its PSD cones, in the caller's cone order).  Rejects what proxsdp_hip_solve_sharded rejects before it
 * starts a thread (PROXSDP_E_INVALID). */
typedef struct proxsdp_shard {
    int64_t struct_size;
    int64_t n, p, m, nnz_A, nnz_G, n_coupling, n_psd, len_psd, n_soc, len_soc, len_eig; /* out: sizes */
    int64_t* vars; int64_t* rows_eq; int64_t* rows_in;                               /* n, p, m */
    int64_t* coupling_rows; int32_t* coupling_owned;                                 /* n_coupling each */
    int64_t* A_colptr; int64_t* A_rowval; double* A_nzval;                           /* n + 1, nnz_A, nnz_A */
    int64_t* G_colptr; int64_t* G_rowval; double* G_nzval;                           /* n + 1, nnz_G, nnz_G */
    double* b; double* h; double* c;                                                 /* p, m, n */
    int64_t* psd_ids; int64_t* psd_ptr; int64_t* psd_idx;                            /* n_psd, n_psd + 1, len_psd */
    int64_t* soc_ids; int64_t* soc_ptr; int64_t* soc_idx;                            /* n_soc, n_soc + 1, len_soc */
    double* eig_resid;                          /* len_eig: the start vectors of the shard's PSD cones (0 without prob->eig_resid) */
} proxsdp_shard;
int proxsdp_host_split_shard(const proxsdp_problem* prob, int32_t n_shards, const int32_t* psd_owner,
                             const int32_t* soc_owner, const int32_t* free_owner, int32_t shard, proxsdp_shard* out);
/* The scalar reduce of an in-process shard group alone: n_shards threads run `rounds` rounds of barrier + combine.
 * records: rounds x n_shards x (nsum + nmax), shard s's packed [sums | maxs] record of round k at
 * records[(k n_shards + s)(nsum + nmax)]; out: n_shards x rounds x (nsum + nmax), what shard s holds after round k.
 * leave_shard >= 0: that thread leaves the group after leave_after completed rounds (the abandon path); every other thread
 * must then come back with an error instead of waiting.  rounds_done[s] = rounds shard s completed, failed[s] = 1 when its
 * next round threw.  timeout_s <= 0: PROXSDP_HIP_COLLECTIVE_TIMEOUT_S (default 300). */
int proxsdp_host_group_reduce(int32_t n_shards, int32_t rounds, int32_t nsum, int32_t nmax, const double* records,
                              int32_t leave_shard, int32_t leave_after, double timeout_s,
                              double* out, int32_t* rounds_done, int32_t* failed);
/* eigen-decomposition of a small dense symmetric matrix (column-major k x k,
 * overwritten by eigenvectors; d ascending) -- the K x K Rayleigh quotient of
 * the thick-restart Lanczos */
int proxsdp_host_symeig(int32_t k, double* a, double* d);
/* the same with the helper threads of the eigenvector accumulation chosen explicitly: 0 = serial,
 * t > 0 = at least t helper threads,
 * -1 = the library's choice (helpers from k >= 96 when PROXSDP_HIP_EIG_THREADS > 0; default 0: they were
 * measured slower on the MI355X host).  Both give bit-identical results. */
int proxsdp_host_symeig_threads(int32_t k, double* a, double* d, int32_t threads);
/* eigen-decomposition of a thick-restarted Rayleigh quotient
 *   T = [diag(D) f 0; f' al[m] be[m] e1'; 0 be[m] e1 tridiag(al[m+1..], be[m+1..])]   (K x K)
 * through the two-phase path the Lanczos driver uses (arrow part reduced first, QL afterwards);
 * U (K x K column-major) eigenvectors, d ascending eigenvalues.  al, be are indexed by step (entries
 * below m unused). */
int proxsdp_host_symeig_arrow(int32_t K, int32_t m, const double* D, const double* f,
                              const double* al, const double* be, double* U, double* d);
/* the same matrix decomposed by a split at k1 and ONE rank-one merge (one level of Cuppen's divide and conquer with
 * Gu-Eisenstat eigenvectors, csrc/host_eig_merge.hpp): what the Lanczos driver uses from krylovdim 64 on, with the first
 * part solved while the GPU still runs the cycle.  k1 = m + 1 when m > 0 (the arrow with its hub), 1 <= k1 < K when
 * m = 0.  info[3] (optional): non-deflated poles, deflated poles, most secular iterations of a root. */
int proxsdp_host_symeig_split(int32_t K, int32_t m, int32_t k1, const double* D, const double* f,
                              const double* al, const double* be, double* U, double* d, int32_t* info);
/* the same with `threads` helper threads for the merge's independent pieces (options.host_merge_threads): bit-identical */
int proxsdp_host_symeig_split_threads(int32_t K, int32_t m, int32_t k1, const double* D, const double* f,
                                      const double* al, const double* be, int32_t threads, double* U, double* d, int32_t* info);
/* The same split with the rank-one merge on the DEVICE (options.device_eig_merge, csrc/merge_device.hip.hpp): first part and
 * tail QL on the host, then the code the Lanczos driver runs -- plan without Qf, packed upload, the merge kernels -- on
 * options-independent defaults (device 0's current context, a stream of its own).  Same outputs as proxsdp_host_symeig_split;
 * PROXSDP_E_INTERNAL when the device hands the merge back.  Needs a HIP device. */
int proxsdp_device_symeig_split(int32_t K, int32_t m, int32_t k1, const double* D, const double* f,
                                const double* al, const double* be, double* U, double* d, int32_t* info);
/* The planner of that merge (Rank1Merge::plan), for tests: the same split, then plan() with (with_qf = 1, what the host merge
 * runs) or without Qf (what the device merge runs).  Q1 (k1 x k1) and Q2 (k2 x k2): the two parts' eigenvectors, column-major;
 * Qf (K x K, written only when with_qf): the assembled and rotated eigenvector matrix in pole order; d, z (K): poles and
 * weights after deflation; colsrc (K): pole p is column colsrc[p] of Q1 when >= 0, else column -(colsrc[p] + 1) of Q2;
 * nd (K): the non-deflated poles, counts[0] of them; rot_idx (2 K) / rot_cs (2 K): the rotations (pj, j) / (c, s) in order,
 * counts[2] of them (x = Qf[:, pj], y = Qf[:, j]: x <- c x + s y, y <- c y - s x); counts[1]: deflated poles. */
int proxsdp_host_merge_plan(int32_t K, int32_t m, int32_t k1, const double* D, const double* f, const double* al,
                            const double* be, int32_t with_qf, double* Q1, double* Q2, double* Qf, double* d, double* z,
                            int32_t* colsrc, int32_t* nd, int32_t* rot_idx, double* rot_cs, int32_t* counts);
/* the library's Lanczos start vector (init 3/2/1 as options.jl:98-103) */
int proxsdp_host_start_vector(int64_t n, int64_t seed, int32_t init, double* out);
/* preprocess!/norm_scaling (scaling.jl): returns the variable order, the
 * inverse permutation and the scaled c; for layout tests */
int proxsdp_host_preprocess(const proxsdp_problem* prob, int64_t* order, int64_t* var_ordering,
                            double* c_scaled, double* frobenius_norm_M);
/* prepare() as proxsdp_hip_model_create runs it, with the position maps it records, and no device: the dump's sizes, norms
 * and arrays as proxsdp_hip_model_dump gives them for a fresh model without equilibration (support = every position whose
 * column is non-empty or whose c is not zero, whatever the auto rule of the support path would decide; ns its length), and
 * for entry q of [A.nzval; G.nzval] its position in csc_val (csc_pos[q]) and in csr_val (csr_pos[q]); nnz_A = entries of A.
 * An array is written when its pointer is not NULL. */
int proxsdp_host_model_prepare(const proxsdp_problem* prob, proxsdp_model_dump* out, int64_t* nnz_A, int32_t* csc_pos,
                               int32_t* csr_pos);
/* the planner proxsdp_hip_model_rows runs, with no device: prob is the model BEFORE the change (as create was given it), ch
 * the change with HOST add_val / add_h.  Out: the dump of the changed model exactly as proxsdp_host_model_prepare gives it
 * for the changed problem; for every position of the new csc_val / csr_val where its value comes from (csc_src / csr_src:
 * q >= 0 = position q of the old array, -1 - t = entry t of add_val); the same map for [b; h'] (bh_src, -1 - t = entry t of
 * add_h); the new position maps csc_pos / csr_pos; ch->kept, m_new, nnz_new.  An array is written when its pointer is not
 * NULL.  Every refusal of proxsdp_hip_model_rows that needs no device applies, with the same codes. */
int proxsdp_host_model_rows_plan(const proxsdp_problem* prob, proxsdp_model_rows* ch, proxsdp_model_dump* out,
                                 int32_t* csc_src, int32_t* csr_src, int32_t* bh_src, int32_t* csc_pos, int32_t* csr_pos);
/* equilibrate! (equilibration.jl) from the row sums alone: rowsums[r] = sum_j M[r,j]^2 of a Q x n matrix in, E (Q) and
 * the scalar d (D = d I: the reference replaces v by its mean in every iteration) out -- the iteration a dense A takes,
 * where M is only streamed.  Uses opt's equilibration_iters / _lb / _ub / _reference_aliasing (NULL: the defaults). */
int proxsdp_host_equilibrate_rowsums(const double* rowsums, int64_t Q, int64_t n, const proxsdp_options* opt,
                                     double* E, double* d);

#ifdef __cplusplus
}
#endif
#endif /* PROXSDP_HIP_H */
