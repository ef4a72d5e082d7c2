"""ctypes binding of include/proxsdp_hip.h (libproxsdp_hip.so).

This is the Python twin of the Julia `ccall` shim in julia/ProxSDPHip.jl: it
marshals the standard form that `_optimize!` builds
(/root/reference/src/MOI_wrapper.jl:229-292) into `proxsdp_problem`, calls
`proxsdp_hip_solve` -- the replacement for `chambolle_pock(aff, con, options)`
at MOI_wrapper.jl:310 -- and copies `proxsdp_result` out.

There is no CPU fallback: a missing library raises ImportError-like
`LibraryNotBuilt`, and every compute entry point raises `ProxSDPHipError` when
the HIP runtime reports no device.
"""
import ctypes as C
import os
import pathlib
import re

import numpy as np
import scipy.sparse as sp

_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = _HERE / "libproxsdp_hip.so"
HEADER_PATH = _HERE.parent / "include" / "proxsdp_hip.h"

TRACE_COLS = 14
TRACE_NAMES = ("iter", "prim_obj", "dual_obj", "gap", "feas", "prim_res", "dual_res",
               "primal_step", "beta", "theta", "target_rank", "trials", "elapsed", "matvecs")


class LibraryNotBuilt(RuntimeError):
    pass


class ProxSDPHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libproxsdp_hip error {code}: {msg}")
        self.code = code


i32, i64, f64 = C.c_int32, C.c_int64, C.c_double
pi64 = C.POINTER(C.c_int64)
pf64 = C.POINTER(C.c_double)


class CSC(C.Structure):
    _fields_ = [("nrows", i64), ("ncols", i64), ("colptr", pi64), ("rowval", pi64), ("nzval", pf64)]


class Problem(C.Structure):
    _fields_ = [("n", i64), ("p", i64), ("m", i64), ("A", CSC), ("G", CSC),
                ("b", pf64), ("h", pf64), ("c", pf64),
                ("n_psd", i64), ("psd_ptr", pi64), ("psd_idx", pi64),
                ("n_soc", i64), ("soc_ptr", pi64), ("soc_idx", pi64),
                ("index_base", i32), ("reserved0", i32), ("eig_resid", pf64),
                ("reduce_ctx", C.c_void_p), ("reduce_fn", C.c_void_p),
                ("M_dense", C.c_void_p), ("M_dense_on_device", i32), ("reserved1", i32),
                ("n_coupling", i64), ("coupling_rows", pi64), ("coupling_owned", C.POINTER(i32)),
                ("reduce_vec_fn", C.c_void_p), ("reduce_vec_on_device", i32), ("reserved2", i32),
                ("nccl_comm", C.c_void_p), ("reserved3", i64)]


REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, pf64, i32, pf64, i32)
REDUCE_VEC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, i64, i32)


def _opt_fields():
    F = []
    a = lambda name, t: F.append((name, t))
    a("struct_size", i64)
    for nme in ("log_verbose", "log_freq", "timer_verbose", "timer_file", "disable_julia_logger",
                "warn_on_limit", "extended_log", "extended_log2", "log_repeat_header", "pad0"):
        a(nme, i32)
    a("time_limit", f64)
    for nme in ("tol_gap", "tol_feasibility", "tol_feasibility_dual", "tol_primal", "tol_dual",
                "tol_psd", "tol_soc"):
        a(nme, f64)
    a("check_dual_feas", i32); a("check_dual_feas_freq", i32)
    a("max_obj", f64); a("min_iter_max_obj", i32); a("pad1", i32)
    a("min_iter_time_infeas", i32); a("pad2", i32)
    for nme in ("infeas_gap_tol", "infeas_limit_gap_tol", "infeas_stable_gap_tol",
                "infeas_feasibility_tol", "infeas_stable_feasibility_tol"):
        a(nme, f64)
    a("certificate_search", i32); a("pad3", i32)
    a("certificate_obj_tol", f64); a("certificate_fail_tol", f64)
    a("min_beta", f64); a("max_beta", f64); a("initial_beta", f64)
    a("initial_adapt_level", f64); a("adapt_decay", f64); a("adapt_window", i32); a("pad4", i32)
    a("convergence_window", i32); a("convergence_check", i32)
    for nme in ("max_iter", "min_iter", "divergence_min_update", "max_iter_lp", "max_iter_conic",
                "max_iter_local"):
        a(nme, i64)
    a("advanced_initialization", i32); a("line_search_flag", i32)
    a("max_linsearch_steps", i32); a("pad5", i32)
    a("delta", f64); a("initial_theta", f64); a("linsearch_decay", f64)
    a("full_eig_decomp", i32); a("max_target_rank_krylov_eigs", i32)
    a("min_size_krylov_eigs", i32); a("warm_start_eig", i32)
    a("rank_increment", i32); a("rank_increment_factor", i32)
    a("eigsolver", i32); a("eigsolver_min_lanczos", i32); a("eigsolver_resid_seed", i64)
    a("arpack_tol", f64); a("arpack_resid_init", i32); a("arpack_reset_resid", i32); a("arpack_max_iter", i64)
    a("krylovkit_reset_resid", i32); a("krylovkit_resid_init", i32)
    a("krylovkit_tol", f64); a("krylovkit_max_iter", i32); a("krylovkit_eager", i32); a("krylovkit_verbose", i32)
    a("reduce_rank", i32); a("rank_slack", i32); a("pad6", i32)
    a("full_eig_freq", i64); a("full_eig_len", i64)
    a("equilibration", i32); a("equilibration_iters", i32)
    a("equilibration_lb", f64); a("equilibration_ub", f64); a("equilibration_limit", f64)
    a("equilibration_force", i32); a("approx_norm", i32)
    a("device_id", i32); a("trace_capacity", i32); a("profile_symv_every", i32); a("support_path", i32)
    a("lanczos_operator", i32); a("initial_target_rank", i32)
    a("full_eig_lanczos", i32); a("lanczos_cycle_kernel", i32); a("lanczos_warm_start", i32)
    a("reconstruct_mfma", i32); a("small_block_batch", i32); a("full_eig_sign", i32); a("psd_sign_engine", i32)
    a("full_eig_lanczos_verify", i32); a("full_eig_lanczos_posres", f64); a("full_eig_lanczos_kdim10", i32)
    a("sign_small_tile_max", i32); a("host_eig_threads", i32); a("block_threads", i32)
    a("host_eig_merge", i32); a("block_batch", i32); a("rocsolver_warmup", i32); a("debug_fail_iteration", i32); a("host_wait_spin", i32)
    a("sign_start_row", i32); a("general_batch", i32); a("full_eig_lanczos_certify", i32); a("host_merge_threads", i32); a("reserved_i", i32 * 1)
    a("full_eig_lanczos_tol", f64); a("reserved_d", f64 * 1)
    a("equilibration_reference_aliasing", i32); a("reserved_i3", i32 * 2)
    a("block_batch_groups", i32); a("lanczos_wide_krylov", i32); a("reserved_i2", i32 * 6); a("device_eig_merge", i32); a("full_eig_lanczos_warm_pow", f64); a("reserved_d2", f64 * 3)
    return F


class Options(C.Structure):
    _fields_ = _opt_fields()


class Stats(C.Structure):
    _fields_ = [("lanczos_matvecs", i64), ("lanczos_restarts", i64), ("lanczos_calls", i64),
                ("full_eigs", i64), ("krylov_fallbacks", i64), ("linesearch_trials", i64),
                ("symv_launches", i64), ("symv_profiled", i64), ("symv_profiled_ms", f64),
                ("symv_bytes", f64), ("algorithmic_bytes", f64), ("init_time", f64),
                ("loop_time", f64), ("exit_time", f64), ("t_primal", f64), ("t_psd", f64),
                ("t_linesearch", f64), ("t_residual", f64), ("dense_passes", i64), ("dense_ms", f64), ("fop_projections", i64), ("exit_matvecs", i64),
                ("host_eig_time", f64), ("host_eigs", i64), ("device_eigs", i64), ("batched_small_eigs", i64),
                ("mfma_reconstructions", i64), ("orth_profiled", i64), ("orth_profiled_ms", f64),
                ("full_eig_solver_ms", f64), ("full_eig_recon_ms", f64), ("cycle_launches", i64),
                ("full_eigs_lanczos", i64), ("cycle_steps", i64), ("cycle_ms", f64), ("warm_starts", i64),
                ("full_eigs_sign", i64), ("sign_products", i64),
                ("sign_engine_projections", i64), ("sign_engine_rejected", i64),
                ("sign_engine_checks", i64), ("sign_engine_mismatches", i64),
                ("full_eigs_lanczos_checks", i64), ("full_eigs_lanczos_mismatches", i64),
                ("batched_block_steps", i64), ("rccl_reductions", i64),
                ("batched_profiled_blocks", i64), ("host_eig_merges", i64),
                ("host_eig_overlap_time", f64), ("sign_short_pass", i64), ("sign_short_fail", i64),
                ("full_eigs_lanczos_certified", i64), ("full_eigs_lanczos_cert_failed", i64), ("cert_matvecs", i64),
                ("dense_truncated_projections", i64), ("wide_krylov_projections", i64), ("reserved_s", i64 * 4),
                ("dense_setup_passes", i64), ("dense_sigma_steps", i64)]


class Result(C.Structure):
    _fields_ = [("status", i32), ("certificate_found", i32), ("primal_feasible_user_tol", i32),
                ("dual_feasible_user_tol", i32), ("result_count", i32), ("final_rank", i32),
                ("iter", i64), ("primal_residual", f64), ("dual_residual", f64),
                ("objval", f64), ("dual_objval", f64), ("gap", f64), ("time", f64),
                ("dual_feasibility", f64),
                ("primal", pf64), ("dual_cone", pf64), ("dual_eq", pf64), ("dual_in", pf64),
                ("slack_eq", pf64), ("slack_in", pf64), ("trace", pf64), ("trace_rows", i64),
                ("status_string", C.c_char * 256), ("stats", Stats)]


# named slots of Stats.reserved_s (include/proxsdp_hip.h PROXSDP_STATS_*): SolveResult.stats lists them under their names
STATS_RESERVED_SLOTS = {"sharded_general_iterations": 0, "device_eig_merges": 1, "device_eig_merge_fallbacks": 2,
                        "fop_owner_steps": 3}

STATE_NHIST = 7
STATE_HIST_NAMES = ("dual_gap", "prim_obj", "dual_obj", "feasibility", "primal_residual", "dual_residual", "comb_residual")
STATE_SCAL_NAMES = ("primal_step", "primal_step_old", "dual_step", "beta", "theta", "adapt_level",
                    "equa_feasibility", "ineq_feasibility", "dual_feasibility")


class State(C.Structure):
    _fields_ = [("struct_size", i64), ("iteration", i64), ("n", i64), ("Q", i64), ("n_psd", i64), ("hist_len", i64),
                ("x", pf64), ("y", pf64), ("Mty", pf64), ("Mx", pf64),
                ("target_rank", pi64), ("current_rank", pi64), ("min_eig", pf64), ("hist", pf64),
                ("scal", f64 * 16), ("ints", i64 * 8)]


class ShardIO(C.Structure):
    """proxsdp_shard (include/proxsdp_hip.h)"""
    _fields_ = ([("struct_size", i64)] +
                [(k, i64) for k in ("n", "p", "m", "nnz_A", "nnz_G", "n_coupling", "n_psd", "len_psd", "n_soc", "len_soc", "len_eig")] +
                [("vars", pi64), ("rows_eq", pi64), ("rows_in", pi64), ("coupling_rows", pi64), ("coupling_owned", C.POINTER(i32)),
                 ("A_colptr", pi64), ("A_rowval", pi64), ("A_nzval", pf64), ("G_colptr", pi64), ("G_rowval", pi64), ("G_nzval", pf64),
                 ("b", pf64), ("h", pf64), ("c", pf64),
                 ("psd_ids", pi64), ("psd_ptr", pi64), ("psd_idx", pi64), ("soc_ids", pi64), ("soc_ptr", pi64), ("soc_idx", pi64), ("eig_resid", pf64)])


class PsdFactors(C.Structure):
    """proxsdp_psd_factors (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("n_psd", i64), ("cap", pi64), ("vec_ptr", pi64), ("val_ptr", pi64),
                ("vectors", pf64), ("values", pf64), ("rank", pi64), ("rank_found", pi64), ("source", C.POINTER(i32)),
                ("resid", pf64), ("xnorm", pf64)]


class Start(C.Structure):
    """proxsdp_start (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("primal", pf64), ("dual_eq", pf64), ("dual_in", pf64), ("n_psd", i64),
                ("rank", pi64), ("vec_ptr", pi64), ("val_ptr", pi64), ("vectors", pf64), ("values", pf64),
                ("target_rank", pi64), ("primal_step", f64), ("beta", f64)]


class DeviceVectors(C.Structure):
    """proxsdp_device_vectors (include/proxsdp_hip.h): device pointers, borrowed and trusted"""
    _fields_ = [("struct_size", i64), ("device_id", i32), ("reserved", i32),
                ("primal", pf64), ("dual_cone", pf64), ("dual_eq", pf64), ("slack_eq", pf64),
                ("dual_in", pf64), ("slack_in", pf64)]


class ModelData(C.Structure):
    """proxsdp_model_data (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("on_device", i32), ("reserved", i32),
                ("c", pf64), ("b", pf64), ("h", pf64), ("A_nzval", pf64), ("G_nzval", pf64)]


class ModelInfo(C.Structure):
    """proxsdp_model_info (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("n", i64), ("p", i64), ("m", i64), ("n_psd", i64), ("nnz", i64),
                ("device_id", i32), ("use_support", i32), ("solves", i64), ("updates", i64), ("support_rebuilds", i64),
                ("device_bytes", i64), ("setup_time", f64)]


class ModelDump(C.Structure):
    """proxsdp_model_dump (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("n", i64), ("Q", i64), ("nnz", i64), ("ns", i64),
                ("csc_val", pf64), ("csr_val", pf64), ("csc_val_orig", pf64), ("csr_val_orig", pf64),
                ("c", pf64), ("c_orig", pf64), ("bh", pf64), ("support", C.POINTER(i32)), ("cS", pf64),
                ("norms", f64 * 4)]


class ModelRows(C.Structure):
    """proxsdp_model_rows (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("on_device", i32), ("reserved", i32),
                ("n_drop", i64), ("drop", pi64), ("n_add", i64), ("add_ptr", pi64), ("add_col", pi64),
                ("add_val", pf64), ("add_h", pf64),
                ("m_new", i64), ("nnz_new", i64), ("kept", pi64), ("support_rebuilt", i32), ("reserved2", i32),
                ("bytes_allocated", i64), ("seconds", f64)]


class TriangleCutsIO(C.Structure):
    """proxsdp_triangle_cuts (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("on_device", i32), ("cone", i32), ("count", i64), ("min_violation", f64),
                ("rhs", f64), ("cand_cap", i64), ("primal", pf64),
                ("tri", pi64), ("pattern", C.POINTER(i32)), ("violation", pf64), ("add_col", pi64), ("add_val", pf64),
                ("add_h", pf64),
                ("n_rows", i64), ("violated", i64), ("scanned", i64), ("passes", i32), ("reserved", i32),
                ("bytes_allocated", i64), ("seconds", f64), ("sweep_seconds", f64)]


class CliqueCutsIO(C.Structure):
    """proxsdp_clique_cuts (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("on_device", i32), ("cone", i32), ("base_size", i32), ("grid", i32), ("batch", i32),
                ("reserved", i32), ("n_base", i64), ("rhs", f64), ("min_violation", f64),
                ("primal", pf64), ("base_nodes", pi64), ("base_sign", C.POINTER(C.c_int8)),
                ("nodes", pi64), ("signs", C.POINTER(C.c_int8)), ("violation", pf64), ("from_base", pi64),
                ("add_col", pi64), ("add_val", pf64), ("add_h", pf64),
                ("n_rows", i64), ("violated_bases", i64), ("scanned", i64), ("bytes_allocated", i64),
                ("seconds", f64), ("sweep_seconds", f64)]


class InactiveRowsIO(C.Structure):
    """proxsdp_inactive_rows (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("on_device", i32), ("reserved", i32), ("dual_in", pf64), ("slack_in", pf64),
                ("dual_tol", f64), ("slack_tol", f64), ("rows", pi64), ("n_rows", i64)]


class RoundingIO(C.Structure):
    """proxsdp_rounding (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("on_device", i32), ("cone", i32), ("r", i32), ("trials", i32), ("seed", i64),
                ("max_sweeps", i32), ("grid_adjacency", i32), ("grid_directions", i32), ("grid_signs", i32),
                ("grid_search", i32), ("lds_side", i32),
                ("V", pf64), ("values", pf64),
                ("signs", C.POINTER(C.c_int8)), ("values_rounded", pf64), ("values_final", pf64),
                ("adj_ptr", pi64), ("adj_col", pi64), ("adj_val", pf64), ("diag", pf64), ("adj_cap", i64),
                ("adj_nnz", i64), ("best_trial", i64), ("value", f64), ("value_rounded", f64), ("flips", i64),
                ("sweeps", i32), ("reserved", i32), ("bytes_allocated", i64), ("seconds", f64), ("search_seconds", f64)]


class DualBoundIO(C.Structure):
    """proxsdp_dual_bound (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("on_device", i32), ("reserved", i32),
                ("dual_eq", pf64), ("dual_in", pf64), ("trace_cap", pf64),
                ("shift", pf64), ("lambda_lower", pf64), ("radius", pf64),
                ("factorisations", C.POINTER(i32)), ("certified", C.POINTER(i32)), ("delta", pf64), ("trace_used", pf64),
                ("bound", f64), ("dual_objective", f64), ("bytes_allocated", i64), ("seconds", f64), ("factor_seconds", f64)]


MODEL_DUMP_ARRAYS = (("csc_val", "nnz"), ("csr_val", "nnz"), ("csc_val_orig", "nnz"), ("csr_val_orig", "nnz"),
                     ("c", "n"), ("c_orig", "n"), ("bh", "Q"), ("support", "ns"), ("cS", "ns"))
MODEL_NORM_NAMES = ("norm_b", "norm_h", "norm_c", "frob")

FACTOR_NONE, FACTOR_RITZ, FACTOR_EIG = 0, 1, 2
FACTOR_SOURCE_NAMES = {FACTOR_NONE: "NONE", FACTOR_RITZ: "RITZ", FACTOR_EIG: "EIG"}


_lib = None


def header_symbols():
    """Every function the public header declares (used by the CPU symbol test)."""
    txt = HEADER_PATH.read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(proxsdp_(?:hip|host)_\w+)\s*\(", txt)))


def lib():
    """Load libproxsdp_hip.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise LibraryNotBuilt(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C proxsdp.jl_amd/csrc`).  There is no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own HIP/HSA runtime.  Measured on the MI355X box: if the
    # system runtime behind this library initialises first, torch can no longer see the GPU
    # ("No HIP GPUs are available"); the other order works, including torch device pointers
    # handed to the library (M_dense).  So when torch is already imported, let it go first.
    import sys
    if "torch" in sys.modules:
        try:
            tc = sys.modules["torch"].cuda
            if tc.is_available():
                tc.init()
        except Exception:
            pass
    L = C.CDLL(str(LIB_PATH))
    L.proxsdp_hip_abi_version.restype = C.c_int
    L.proxsdp_hip_last_error.restype = C.c_char_p
    L.proxsdp_hip_default_options.argtypes = [C.POINTER(Options)]
    L.proxsdp_hip_default_options.restype = None
    L.proxsdp_hip_set_option.argtypes = [C.POINTER(Options), C.c_char_p, f64]
    L.proxsdp_hip_get_option.argtypes = [C.POINTER(Options), C.c_char_p, pf64]
    L.proxsdp_hip_solve.argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(Result)]
    L.proxsdp_hip_solve_ex.argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(Result),
                                       C.POINTER(State), C.POINTER(State)]
    L.proxsdp_hip_solve_factored.argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(Result),
                                             C.POINTER(PsdFactors)]
    L.proxsdp_hip_solve_from.argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(Result),
                                         C.POINTER(Start), C.POINTER(PsdFactors)]
    L.proxsdp_hip_start_point.argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(Start), C.POINTER(State)]
    L.proxsdp_hip_solve_device.argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(Result), C.POINTER(Start),
                                           C.POINTER(DeviceVectors), C.POINTER(PsdFactors), C.POINTER(DeviceVectors)]
    L.proxsdp_hip_exit_vectors.argtypes = [C.POINTER(Problem), C.POINTER(Options), pf64, pf64, i32] + [pf64] * 8 + [i64]
    L.proxsdp_hip_model_create.argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(C.c_void_p)]
    L.proxsdp_hip_model_update.argtypes = [C.c_void_p, C.POINTER(ModelData)]
    L.proxsdp_hip_model_solve.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(Result), C.POINTER(Start),
                                          C.POINTER(DeviceVectors), C.POINTER(PsdFactors), C.POINTER(DeviceVectors)]
    L.proxsdp_hip_model_info.argtypes = [C.c_void_p, C.POINTER(ModelInfo)]
    L.proxsdp_hip_model_destroy.argtypes = [C.c_void_p]
    L.proxsdp_hip_model_dump.argtypes = [C.c_void_p, C.POINTER(ModelDump)]
    L.proxsdp_hip_model_norm2.argtypes = [pf64, i64, i32, pf64]
    L.proxsdp_host_model_prepare.argtypes = [C.POINTER(Problem), C.POINTER(ModelDump), pi64, C.POINTER(i32), C.POINTER(i32)]
    L.proxsdp_hip_model_rows.argtypes = [C.c_void_p, C.POINTER(ModelRows)]
    L.proxsdp_host_model_rows_plan.argtypes = [C.POINTER(Problem), C.POINTER(ModelRows), C.POINTER(ModelDump)] + [C.POINTER(i32)] * 5
    L.proxsdp_hip_model_triangles.argtypes = [C.c_void_p, C.POINTER(TriangleCutsIO)]
    L.proxsdp_host_triangle_cuts.argtypes = [pf64, i64, pi64, i32, C.POINTER(TriangleCutsIO)]
    L.proxsdp_hip_model_inactive_rows.argtypes = [C.c_void_p, C.POINTER(InactiveRowsIO)]
    L.proxsdp_hip_model_cliques.argtypes = [C.c_void_p, C.POINTER(CliqueCutsIO)]
    L.proxsdp_host_clique_cuts.argtypes = [pf64, i64, pi64, i32, C.POINTER(CliqueCutsIO)]
    L.proxsdp_hip_model_round.argtypes = [C.c_void_p, C.POINTER(RoundingIO)]
    L.proxsdp_host_round.argtypes = [i64, pi64, pi64, pf64, pf64, C.POINTER(RoundingIO)]
    L.proxsdp_host_round_directions.argtypes = [i64, i32, i32, pf64]
    L.proxsdp_hip_model_bound.argtypes = [C.c_void_p, C.POINTER(DualBoundIO)]
    L.proxsdp_host_dual_bound.argtypes = [i64, i64, i64, pf64, C.POINTER(CSC), pf64, i64, pi64, pi64, i32, C.POINTER(DualBoundIO)]
    L.proxsdp_hip_cholesky.argtypes = [pf64, i64, f64, pf64, pi64]
    L.proxsdp_host_cholesky.argtypes = [pf64, i64, f64, pf64, pi64]
    L.proxsdp_hip_factor_residual.argtypes = [pf64, i64, pf64, i64, pf64, i32, pf64, pf64]
    L.proxsdp_hip_factor_residual_kernel.argtypes = [pf64, i64, pf64, i64, pf64, i32, pf64, pf64, i32, pf64]
    L.proxsdp_hip_psd_project.argtypes = [pf64, i64, i32, i32, C.POINTER(Options), pf64, pf64,
                                          C.POINTER(i32), pf64, pi64, C.POINTER(i32), C.POINTER(i32)]
    L.proxsdp_hip_eigsolve.argtypes = [pf64, i64, i32, C.POINTER(Options), pf64, i32, pf64, pf64,
                                       C.POINTER(i32), C.POINTER(i32), pi64, C.POINTER(i32)]
    L.proxsdp_hip_symv_packed.argtypes = [pf64, i64, pf64, pf64, i32, pf64]
    L.proxsdp_hip_reconstruct.argtypes = [pf64, pf64, i64, i32, pf64, i32, pf64]
    L.proxsdp_hip_reconstruct_kernel.argtypes = [pf64, pf64, i64, i32, i32, pf64, i32, pf64]
    L.proxsdp_hip_full_eig_kernel.argtypes = [pf64, i64, i32, pf64, i32, pf64, C.POINTER(i32), C.POINTER(i64)]
    L.proxsdp_hip_spmv.argtypes = [C.POINTER(CSC), i32, i32, pf64, pf64]
    L.proxsdp_host_symeig.argtypes = [i32, pf64, pf64]
    L.proxsdp_host_start_vector.argtypes = [i64, i64, i32, pf64]
    L.proxsdp_host_preprocess.argtypes = [C.POINTER(Problem), pi64, pi64, pf64, pf64]
    L.proxsdp_hip_dense_scaling.argtypes = [C.POINTER(Problem), C.POINTER(Options), pf64, pf64, pf64, pf64, C.POINTER(i32)]
    L.proxsdp_host_equilibrate_rowsums.argtypes = [pf64, i64, i64, C.POINTER(Options), pf64, pf64]
    L.proxsdp_hip_project_cones.argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(ProjectConesIO)]
    L.proxsdp_hip_sym_product.argtypes = [C.POINTER(SymProductIO)]
    L.proxsdp_hip_sign_unpack.argtypes = [pf64, i64, f64, pf64, pf64]
    L.proxsdp_hip_reconstruct_fused.argtypes = [C.POINTER(ReconstructFusedIO)]
    L.proxsdp_hip_rotate.argtypes = [C.POINTER(RotationIO)]
    L.proxsdp_hip_tail_copy.argtypes = [C.POINTER(TailCopyIO)]
    L.proxsdp_hip_lanczos_cycles.argtypes = [C.POINTER(LanczosCyclesIO)]
    L.proxsdp_hip_operator_cycles.argtypes = [C.POINTER(OperatorCyclesIO)]
    L.proxsdp_host_block1_lds_doubles.argtypes = [i32, i32, i64, i32]
    L.proxsdp_host_block1_lds_doubles.restype = i64
    L.proxsdp_hip_solve_sharded.argtypes = [C.POINTER(Problem), C.POINTER(Options), i32, C.POINTER(i32), C.POINTER(i32),
                                            C.POINTER(i32), C.POINTER(i32), C.POINTER(Result), C.POINTER(Stats)]
    L.proxsdp_host_split_shard.argtypes = [C.POINTER(Problem), i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32,
                                           C.POINTER(ShardIO)]
    L.proxsdp_host_group_reduce.argtypes = [i32, i32, i32, i32, pf64, i32, i32, f64, pf64, C.POINTER(i32), C.POINTER(i32)]
    L.proxsdp_hip_coupling_sum.argtypes = [pf64, i32, i64, pi64, pf64, i64, pf64]
    L.proxsdp_hip_rccl_unique_id.argtypes = [C.c_void_p]
    L.proxsdp_hip_rccl_comm_init.argtypes = [i32, C.c_void_p, i32, i32, C.POINTER(C.c_void_p)]
    L.proxsdp_hip_rccl_comm_destroy.argtypes = [C.c_void_p]
    if L.proxsdp_hip_abi_version() != 10:
        raise ProxSDPHipError(-1, "ABI version mismatch")
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise ProxSDPHipError(rc, lib().proxsdp_hip_last_error().decode(errors="replace"))


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _p(a, t=pf64):
    return a.ctypes.data_as(t)


def default_options():
    o = Options()
    lib().proxsdp_hip_default_options(C.byref(o))
    return o


def set_option(o, name, value):
    """RawOptimizerAttribute semantics (MOI_wrapper.jl:84-93): unknown name is an error."""
    rc = lib().proxsdp_hip_set_option(C.byref(o), name.encode(), float(value))
    if rc != 0:
        raise KeyError(f"No parameter matching {name}")


def get_option(o, name):
    v = f64()
    rc = lib().proxsdp_hip_get_option(C.byref(o), name.encode(), C.byref(v))
    if rc != 0:
        raise KeyError(f"No parameter matching {name}")
    return v.value


def device_count():
    return lib().proxsdp_hip_device_count()


class _Marshalled:
    """Keeps the numpy arrays behind a proxsdp_problem alive."""

    def __init__(self, prob, eig_resid=None, index_base=0):
        """index_base = 1 hands the library what Julia's ccall hands it: 1-based Int64 colptr / rowval
        (SparseMatrixCSC, structs.jl:36-37) and 1-based cone variable lists (SDPSet.vec_i, SOCSet.idx,
        structs.jl:44-53); the offsets psd_ptr / soc_ptr stay 0-based (julia/ProxSDPHip.jl)."""
        if index_base not in (0, 1):
            raise ValueError("index_base must be 0 or 1")
        keep = []

        def csc(M, ncols):
            M = sp.csc_matrix(M, dtype=np.float64)
            M.sort_indices()
            cp, rv, nz = _i(M.indptr) + index_base, _i(M.indices) + index_base, _f(M.data)
            keep.extend([cp, rv, nz])
            return CSC(M.shape[0], ncols, _p(cp, pi64), _p(rv, pi64), _p(nz))

        P = Problem()
        P.n, P.p, P.m = prob.n, prob.A.shape[0], prob.G.shape[0]
        P.A, P.G = csc(prob.A, prob.n), csc(prob.G, prob.n)
        b, h, c = _f(prob.b), _f(prob.h), _f(prob.c)
        keep.extend([b, h, c])
        P.b, P.h, P.c = _p(b), _p(h), _p(c)

        def cones(lst):
            ptr = np.zeros(len(lst) + 1, dtype=np.int64)
            for k, v in enumerate(lst):
                ptr[k + 1] = ptr[k] + len(v)
            idx = (_i(np.concatenate(lst)) + index_base) if lst else np.zeros(1, dtype=np.int64)
            keep.extend([ptr, idx])
            return len(lst), _p(ptr, pi64), _p(idx, pi64)

        P.n_psd, P.psd_ptr, P.psd_idx = cones(list(prob.psd))
        P.n_soc, P.soc_ptr, P.soc_idx = cones(list(prob.soc))
        P.index_base = index_base
        if eig_resid is not None:
            r = _f(np.concatenate([np.asarray(v, float).ravel() for v in eig_resid]))
            keep.append(r)
            P.eig_resid = _p(r)
        Md = getattr(prob, "M_dense", None)
        if Md is not None:
            if prob.A.nnz:
                raise ValueError("M_dense given: the sparse A must have no stored entries")
            if hasattr(Md, "data_ptr"):                      # torch tensor on the GPU
                if not (Md.is_cuda and Md.is_contiguous() and Md.dtype.is_floating_point and Md.element_size() == 8):
                    raise ValueError("M_dense tensor must be a contiguous float64 CUDA tensor")
                if tuple(Md.shape) != (P.p, P.n):
                    raise ValueError("M_dense has the wrong shape")
                P.M_dense, P.M_dense_on_device = Md.data_ptr(), 1
            else:
                Md = np.ascontiguousarray(Md, dtype=np.float64)
                if Md.shape != (P.p, P.n):
                    raise ValueError("M_dense has the wrong shape")
                P.M_dense, P.M_dense_on_device = Md.ctypes.data, 0
            keep.append(Md)
        self.P, self.keep = P, keep


class SolveResult:
    """Result (structs.jl:60-81) copied out of proxsdp_result."""

    def __init__(self, R, n, p, m, arrays, trace):
        for name, _ in Result._fields_:
            if name in ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in", "trace", "stats"):
                continue
            v = getattr(R, name)
            setattr(self, name, v.decode(errors="replace") if isinstance(v, bytes) else v)
        self.primal, self.dual_cone, self.dual_eq, self.dual_in, self.slack_eq, self.slack_in = arrays
        self.stats = {k: (list(getattr(R.stats, k)) if k.startswith("reserved") else getattr(R.stats, k))
                      for k, _ in Stats._fields_}
        for k, slot in STATS_RESERVED_SLOTS.items():
            self.stats[k] = int(R.stats.reserved_s[slot])
        self.trace = trace[:R.trace_rows].copy()
        for k in ("certificate_found", "primal_feasible_user_tol", "dual_feasible_user_tol"):
            setattr(self, k, bool(getattr(self, k)))

    def trace_dicts(self):
        return [dict(zip(TRACE_NAMES, row)) for row in self.trace]


def rccl_available():
    return lib().proxsdp_hip_rccl_available() == 1


def rccl_unique_id():
    """128 bytes from ncclGetUniqueId (one rank calls this and ships the bytes to the others)."""
    buf = C.create_string_buffer(128)
    _check(lib().proxsdp_hip_rccl_unique_id(buf))
    return bytes(buf.raw)


def rccl_comm_init(nranks, uid, rank, device_id=0):
    """ncclCommInitRank through the library's librccl; returns the opaque communicator handle (int)."""
    comm = C.c_void_p()
    buf = C.create_string_buffer(bytes(uid), 128)
    _check(lib().proxsdp_hip_rccl_comm_init(int(nranks), buf, int(rank), int(device_id), C.byref(comm)))
    return comm.value


def rccl_comm_destroy(comm):
    if comm:
        _check(lib().proxsdp_hip_rccl_comm_destroy(C.c_void_p(comm)))


def _state_struct(n, Q, n_psd, window, state=None, iteration=0):
    """proxsdp_state over fresh numpy arrays (filled from the dict `state` when given).  Returns (struct, arrays)."""
    hl = 2 * int(window)
    arr = dict(x=np.zeros(max(n, 1)), y=np.zeros(max(Q, 1)), Mty=np.zeros(max(n, 1)), Mx=np.zeros(max(Q, 1)),
               target_rank=np.zeros(max(n_psd, 1), dtype=np.int64), current_rank=np.zeros(max(n_psd, 1), dtype=np.int64),
               min_eig=np.zeros(max(n_psd, 1)), hist=np.zeros((STATE_NHIST, hl)))
    S = State()
    S.struct_size = C.sizeof(State)
    S.iteration, S.n, S.Q, S.n_psd, S.hist_len = int(iteration), n, Q, n_psd, hl
    if state is not None:
        S.iteration = int(state["iteration"])
        for k in ("x", "y", "Mty", "Mx", "min_eig"):
            v = _f(state[k]).ravel()
            if len(v) != {"x": n, "Mty": n, "y": Q, "Mx": Q, "min_eig": n_psd}[k]:
                raise ValueError(f"state[{k!r}] has the wrong length")
            arr[k][:len(v)] = v
        for k in ("target_rank", "current_rank"):
            v = _i(state[k]).ravel()
            if len(v) != n_psd:
                raise ValueError(f"state[{k!r}] has the wrong length")
            arr[k][:len(v)] = v
        h = np.asarray(state["hist"], dtype=np.float64)
        if h.shape != (STATE_NHIST, hl):
            raise ValueError("state['hist'] must be 7 x 2*convergence_window")
        arr["hist"][:] = h
        for q, nme in enumerate(STATE_SCAL_NAMES):
            S.scal[q] = float(state[nme])
        S.ints[0], S.ints[1], S.ints[2] = int(state["rank_update"]), int(state["update_cont"]), int(state["ada_count"])
    S.x, S.y, S.Mty, S.Mx = _p(arr["x"]), _p(arr["y"]), _p(arr["Mty"]), _p(arr["Mx"])
    S.target_rank, S.current_rank = _p(arr["target_rank"], pi64), _p(arr["current_rank"], pi64)
    S.min_eig, S.hist = _p(arr["min_eig"]), _p(arr["hist"])
    return S, arr


def _state_dict(S, arr, n, Q, n_psd):
    d = dict(iteration=int(S.iteration), x=arr["x"][:n].copy(), y=arr["y"][:Q].copy(), Mty=arr["Mty"][:n].copy(),
             Mx=arr["Mx"][:Q].copy(), target_rank=arr["target_rank"][:n_psd].copy(),
             current_rank=arr["current_rank"][:n_psd].copy(), min_eig=arr["min_eig"][:n_psd].copy(),
             hist=arr["hist"].copy(), rank_update=int(S.ints[0]), update_cont=int(S.ints[1]), ada_count=int(S.ints[2]))
    for q, nme in enumerate(STATE_SCAL_NAMES):
        d[nme] = float(S.scal[q])
    return d


def psd_sides(prob):
    """side of every PSD cone of `prob`, in cone order"""
    return [int(round((np.sqrt(8.0 * len(v) + 1.0) - 1.0) / 2.0)) for v in prob.psd]


def _factors_struct(sides, factors):
    """proxsdp_psd_factors for cones of the given sides, and the arrays behind it.  factors: True = room for every pair of
    every cone (cap = side), or {cone number: cap} (cones not named: cap 0, nothing computed for them)."""
    nb = len(sides)
    if factors is True:
        cap = np.array(sides, dtype=np.int64).reshape(nb)
    else:
        cap = np.zeros(nb, dtype=np.int64)
        for k, c in dict(factors).items():
            if not 0 <= int(k) < nb:
                raise ValueError(f"factors: no PSD cone {k}")
            if int(c) < 0:
                raise ValueError("factors: negative cap")
            cap[int(k)] = min(int(c), sides[int(k)])           # (a block has at most `side` pairs)
    vec_ptr = np.zeros(nb + 1, dtype=np.int64)
    val_ptr = np.zeros(nb + 1, dtype=np.int64)
    for k in range(nb):
        vec_ptr[k + 1] = vec_ptr[k] + sides[k] * cap[k]
        val_ptr[k + 1] = val_ptr[k] + cap[k]
    arr = dict(cap=cap, vec_ptr=vec_ptr, val_ptr=val_ptr,
               vectors=np.full(max(int(vec_ptr[-1]), 1), np.nan), values=np.full(max(int(val_ptr[-1]), 1), np.nan),
               rank=np.zeros(max(nb, 1), dtype=np.int64), rank_found=np.zeros(max(nb, 1), dtype=np.int64),
               source=np.zeros(max(nb, 1), dtype=np.int32), resid=np.zeros(max(nb, 1)), xnorm=np.zeros(max(nb, 1)))
    F = PsdFactors()
    F.struct_size = C.sizeof(PsdFactors)
    F.n_psd = nb
    F.cap, F.vec_ptr, F.val_ptr = _p(cap, pi64), _p(vec_ptr, pi64), _p(val_ptr, pi64)
    F.vectors, F.values = _p(arr["vectors"]), _p(arr["values"])
    F.rank, F.rank_found = _p(arr["rank"], pi64), _p(arr["rank_found"], pi64)
    F.source = arr["source"].ctypes.data_as(C.POINTER(i32))
    F.resid, F.xnorm = _p(arr["resid"]), _p(arr["xnorm"])
    return F, arr


def _factors_list(sides, arr):
    """[(values, vectors, info)] per PSD cone: values (rank,) descending, vectors (side, rank), info = dict(rank, rank_found,
    source, source_name, resid, xnorm, cap)"""
    out = []
    for k, sd in enumerate(sides):
        r = int(arr["rank"][k])
        vals = arr["values"][arr["val_ptr"][k]:arr["val_ptr"][k] + r].copy()
        vecs = arr["vectors"][arr["vec_ptr"][k]:arr["vec_ptr"][k] + sd * r].reshape(r, sd).T.copy()
        src = int(arr["source"][k])
        out.append((vals, vecs, dict(rank=r, rank_found=int(arr["rank_found"][k]), source=src,
                                     source_name=FACTOR_SOURCE_NAMES.get(src, "?"), resid=float(arr["resid"][k]),
                                     xnorm=float(arr["xnorm"][k]), cap=int(arr["cap"][k]))))
    return out


START_KEYS = ("primal", "dual_eq", "dual_in", "factors", "target_rank", "primal_step", "beta")
DEVICE_START_KEYS = ("primal", "dual_eq", "dual_in")


def _is_tensor(v):
    """a torch tensor (torch is imported only by callers who hand one in, or who ask for device_out)"""
    return hasattr(v, "data_ptr") and hasattr(v, "is_cuda")


def _start_on_device(start):
    """does this start (None, a dict or a SolveResult) hold a CUDA tensor?"""
    if start is None:
        return False
    get = (lambda k: getattr(start, k, None)) if isinstance(start, SolveResult) else dict(start).get
    return any(_is_tensor(get(k)) and get(k).is_cuda for k in DEVICE_START_KEYS)


def _device_ptr(t, length, device_id, what):
    """the device pointer of a float64 CUDA tensor of `length` entries on cuda:device_id, as a POINTER(c_double)"""
    if not (t.is_cuda and t.is_contiguous() and t.dtype.is_floating_point and t.element_size() == 8):
        raise ValueError(f"{what} must be a contiguous float64 CUDA tensor")
    if t.numel() != length:
        raise ValueError(f"{what} must have length {length}")
    if t.device.index != device_id:
        raise ValueError(f"{what} is on {t.device}, the solve runs on cuda:{device_id}")
    return C.cast(C.c_void_p(t.data_ptr() if length else 0), pf64)


def _device_vectors(device_id, **tensors):
    """proxsdp_device_vectors over (tensor, length) pairs; the tensors must outlive the call"""
    D = DeviceVectors()
    D.struct_size = C.sizeof(DeviceVectors)
    D.device_id = device_id
    for k, (t, ln) in tensors.items():
        if t is not None and ln > 0:
            setattr(D, k, _device_ptr(t, ln, device_id, k))
    return D


def _split_device_start(start, n, p, m, device_id):
    """(host part of a start, proxsdp_device_vectors of its CUDA tensors or None, the tensors)"""
    if isinstance(start, SolveResult):
        start = start_from_result(start)
    start = dict(start)
    dev = {k: start.pop(k) for k in DEVICE_START_KEYS if _is_tensor(start.get(k)) and start[k].is_cuda}
    for k in DEVICE_START_KEYS:                              # (a CPU tensor is a host array)
        if _is_tensor(start.get(k)):
            start[k] = start[k].numpy()
    if not dev:
        return start, None, dev
    ln = dict(primal=n, dual_eq=p, dual_in=m)
    return start, _device_vectors(device_id, **{k: (v, ln[k]) for k, v in dev.items()}), dev


def start_from_result(res):
    """The start dictionary of a previous SolveResult: its primal and duals, and -- when the solve returned them
    (solve(factors=...)) -- the factors of every PSD cone.  A cone whose factors were cut by `cap` (info["rank_found"] >
    info["rank"]) or that asked for none (cap 0) gets None: it starts from its entries of `primal`."""
    if _is_tensor(res.dual_eq):                              # a device result (solve(device_out=True)): the tensors as they are
        d = dict(primal=res.primal, dual_eq=res.dual_eq, dual_in=res.dual_in)
    else:
        d = dict(primal=None if res.primal is None else np.array(res.primal, dtype=np.float64),
                 dual_eq=np.array(res.dual_eq, dtype=np.float64), dual_in=np.array(res.dual_in, dtype=np.float64))
    fl = getattr(res, "psd_factors", None)
    if fl is not None:
        fac = []
        for vals, vecs, info in fl:
            cut = info["rank_found"] > info["rank"] or info.get("cap", 1) <= 0
            fac.append(None if cut else (np.array(vals, dtype=np.float64), np.array(vecs, dtype=np.float64)))
        if d["primal"] is None and any(f is None for f in fac):
            raise ValueError("start: a cone without complete factors needs the result's primal (solve(primal=True))")
        d["factors"] = fac
    return d


def _start_struct(n, p, m, sides, start):
    """proxsdp_start for a model with n variables, p + m rows and PSD cones of the given sides, and the arrays behind it.
    start: a dict with any of START_KEYS, or a previous SolveResult (start_from_result).  factors: one entry per PSD cone,
    (values, vectors[, info]) with vectors of shape (side, rank), or None = no factors for that cone."""
    if isinstance(start, SolveResult):
        start = start_from_result(start)
    start = dict(start)
    unknown = set(start) - set(START_KEYS)
    if unknown:
        raise ValueError(f"start: unknown keys {sorted(unknown)}")
    nb = len(sides)
    S = Start()
    S.struct_size = C.sizeof(Start)
    arr = {}
    for k, ln in (("primal", n), ("dual_eq", p), ("dual_in", m)):
        v = start.get(k)
        if v is None:
            continue
        v = _f(v).ravel()
        if len(v) != ln:
            raise ValueError(f"start[{k!r}] must have length {ln}")
        arr[k] = v if len(v) else np.zeros(1)
        setattr(S, k, _p(arr[k]))
    fac = start.get("factors")
    if fac is not None:
        fac = list(fac)
        if len(fac) != nb:
            raise ValueError(f"start['factors'] must have one entry per PSD cone ({nb})")
        rank = np.full(max(nb, 1), -1, dtype=np.int64)
        vec_ptr, val_ptr = np.zeros(nb + 1, dtype=np.int64), np.zeros(nb + 1, dtype=np.int64)
        vecs, vals = [], []
        for k, f in enumerate(fac):
            if f is not None:
                lam, V = _f(f[0]).ravel(), np.asarray(f[1], dtype=np.float64)
                V = V.reshape(sides[k], -1) if V.size else np.zeros((sides[k], 0))
                if V.shape != (sides[k], len(lam)):
                    raise ValueError(f"start['factors'][{k}]: vectors must be (side, rank) = ({sides[k]}, {len(lam)})")
                rank[k] = len(lam)
                vecs.append(V.ravel(order="F")); vals.append(lam)
            vec_ptr[k + 1] = vec_ptr[k] + (sides[k] * rank[k] if rank[k] > 0 else 0)
            val_ptr[k + 1] = val_ptr[k] + max(int(rank[k]), 0)
        arr.update(rank=rank, vec_ptr=vec_ptr, val_ptr=val_ptr,
                   vectors=_f(np.concatenate(vecs + [np.zeros(1)])), values=_f(np.concatenate(vals + [np.zeros(1)])))
        S.n_psd = nb
        S.rank, S.vec_ptr, S.val_ptr = _p(rank, pi64), _p(vec_ptr, pi64), _p(val_ptr, pi64)
        S.vectors, S.values = _p(arr["vectors"]), _p(arr["values"])
    tr = start.get("target_rank")
    if tr is not None:
        tr = _i(tr).ravel()
        if len(tr) != nb:
            raise ValueError(f"start['target_rank'] must have one entry per PSD cone ({nb})")
        arr["target_rank"] = tr if len(tr) else np.zeros(1, dtype=np.int64)
        S.target_rank = _p(arr["target_rank"], pi64)
    S.primal_step = float(start.get("primal_step") or 0.0)
    S.beta = float(start.get("beta") or 0.0)
    return S, arr


def _ref(x):
    return C.byref(x) if x is not None else None


class _SolveCall:
    """What ONE call into a solve entry marshals beside problem and options, and the SolveResult made of it afterwards: the
    proxsdp_result with its trace, the six vectors as host arrays or (device_out) as tensors on cuda:<o.device_id>, the start
    split into its host part and its CUDA tensors, the factors struct.  R, st, sd, F, out are what the entry takes (byref,
    or None where nothing was asked for); run() makes the call.  torch is imported only when tensors are involved."""

    def __init__(self, n, p, m, sides, o, start=None, factors=False, primal=True, device_out=False):
        self.dims, self.sides, self.dev_id = (n, p, m), sides, int(o.device_id)
        lens = (n, n, p, m, p, m)
        self.trace = np.zeros((max(o.trace_capacity, 1), TRACE_COLS))
        self._R = Result()
        self._R.trace = _p(self.trace)
        self.torch = None
        if device_out or _start_on_device(start):
            import torch
            self.torch = torch
        self._keep = []                                      # what the structs point to
        out = None
        if device_out:
            self.arrays = [self.torch.empty(k, dtype=self.torch.float64, device=f"cuda:{self.dev_id}") for k in lens]
            if not primal:
                self.arrays[0] = None
            names = ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in")
            out = _device_vectors(self.dev_id, **{nm: (t, k) for nm, t, k in zip(names, self.arrays, lens)})
        else:
            host = [np.zeros(max(k, 1)) for k in lens]
            R = self._R
            R.primal, R.dual_cone, R.dual_eq, R.dual_in, R.slack_eq, R.slack_in = [_p(a) for a in host]
            self.arrays = [a[:k] for a, k in zip(host, lens)]
            if not primal:
                R.primal = self.arrays[0] = None
        st = sd = F = self._farr = None
        if start is not None:
            hstart, sd, dev = _split_device_start(start, n, p, m, self.dev_id)
            st, sarr = _start_struct(n, p, m, sides, hstart)
            self._keep += [dev, sarr]
        if factors is not False and factors is not None:
            F, self._farr = _factors_struct(sides, factors)
        self._structs = (st, sd, F, out)
        self.R, self.st, self.sd, self.F, self.out = C.byref(self._R), _ref(st), _ref(sd), _ref(F), _ref(out)

    def run(self, entry, *args):
        if self.torch is not None:
            self.torch.cuda.synchronize(self.dev_id)         # the library runs on its own stream
        _check(entry(*args))
        res = SolveResult(self._R, *self.dims, self.arrays, self.trace)
        if self._farr is not None:
            res.psd_factors = _factors_list(self.sides, self._farr)
        return res


def start_point(prob, options=None, start=None, index_base=0, eig_resid=None):
    """proxsdp_hip_start_point: the "Init" section and the start path of a warm-started solve, nothing more.  Returns the
    solver's internal x, Mty (n), y, Mx (p + m), target_rank, the scalars primal_step, primal_step_old, dual_step, beta,
    theta, adapt_level and iteration = 0.  start = None: the cold point."""
    L = lib()
    o = options if options is not None else default_options()
    M = _Marshalled(prob, eig_resid, index_base)
    n, Q, nb = int(M.P.n), int(M.P.p + M.P.m), int(M.P.n_psd)
    st = None
    if start is not None:
        st, sarr = _start_struct(n, int(M.P.p), int(M.P.m), psd_sides(prob), start)
    S, arr = _state_struct(n, Q, nb, o.convergence_window)
    _check(L.proxsdp_hip_start_point(C.byref(M.P), C.byref(o), C.byref(st) if st is not None else None, C.byref(S)))
    d = dict(iteration=int(S.iteration), x=arr["x"][:n].copy(), y=arr["y"][:Q].copy(), Mty=arr["Mty"][:n].copy(),
             Mx=arr["Mx"][:Q].copy(), target_rank=arr["target_rank"][:nb].copy())
    for q, nme in enumerate(STATE_SCAL_NAMES[:6]):
        d[nme] = float(S.scal[q])
    return d


def solve(prob, options=None, eig_resid=None, trace_capacity=0, reduce=None, coupling=None, index_base=0, nccl_comm=None,
          resume=None, capture_iteration=None, factors=False, primal=True, start=None, device_out=False):
    """proxsdp_hip_solve: replaces chambolle_pock(aff, con, options) (MOI_wrapper.jl:310).
    Returns the minimisation objective; sign/constant fix-up is the caller's
    (MOI_wrapper.jl:336-337), see optimizer.Optimizer.
    reduce: optional callable(sums: np.ndarray, maxs: np.ndarray) -> None that all-reduces
    the two arrays in place over the shards of a block-sharded solve (see sharded.py).
    coupling: optional dict(rows=int64 array of this shard's row numbers, owned=int32 0/1 array,
    reduce_vec=callable(ptr: int, length: int, on_device: bool) -> None summing the buffer in place over
    the shards, on_device=bool) -- the rows shared with other shards (proxsdp_problem.coupling_rows).
    nccl_comm: optional RCCL communicator handle (rccl_comm_init): the library then reduces the scalar record and
    the coupling rows itself on its own stream (proxsdp_problem.nccl_comm); `reduce` / reduce_vec are not used.
    resume: optional state dict (as returned in `.state`, or by oracle.export_state) -- the solve continues with iteration
    state['iteration'] + 1 (proxsdp_hip_solve_ex); capture_iteration: k >= 1 -- the state after iteration k comes back as
    `.state` (None when the solve ended before k).  Vectors are in the solver's internal order and scaling.
    factors: True or {cone number: cap} -- proxsdp_hip_solve_factored: the same solve, and `.psd_factors` = one
    (values, vectors, info) per PSD cone with X_k ~ vectors diag(values) vectors' (values descending and > 0; info: rank,
    rank_found, source / source_name, resid, xnorm, cap); True asks for every pair, a dict caps the columns per cone (cones
    it does not name get nothing).  Not with resume / capture_iteration, and not for a shard.
    primal = False: proxsdp_result.primal = NULL (`.primal` comes back None).
    start: warm start (proxsdp_hip_solve_from) -- a dict with any of primal, dual_eq, dual_in (as a result holds them),
    factors = [(values, vectors) | None per PSD cone], target_rank (per cone, 0 = derive), primal_step, beta; or a previous
    SolveResult, whose psd_factors are used when it has them (a cone cut by `cap` starts from its primal entries).  The
    loop is entered at iteration 1 from that point, each factored cone at target rank rank + 1 unless target_rank says
    otherwise.  Combines with factors=; not with resume / capture_iteration / reduce / coupling / nccl_comm.
    device_out = True: proxsdp_hip_solve_device -- the same solve with the exit path on the device; the six vectors of the
    result are float64 torch tensors on cuda:<options.device_id> (in the caller's order and units, the values the arrays
    would hold).  start= then also takes CUDA tensors for primal, dual_eq, dual_in, and a device result as it is, so
    solve(p2, start=solve(p1, device_out=True, factors=True), device_out=True) chains with no n-vector on the host.  The
    library works on its own stream: the device is synchronised before tensors are handed in, and the call returns after
    its writes have completed.  Not with resume / capture_iteration / reduce / coupling / nccl_comm."""
    on_device = device_out or _start_on_device(start)        # proxsdp_hip_solve_device: tensors out and / or in
    if on_device:
        if resume is not None or capture_iteration is not None or reduce is not None or coupling is not None or nccl_comm:
            raise ValueError("device vectors cannot be combined with the state seam or a block-sharded solve")
        import torch                                         # (lazily: the host paths do not need it; before lib(), see there)
    L = lib()
    if on_device and not torch.cuda.is_available():
        raise RuntimeError("torch sees no GPU: import torch before the first call into the library (see binding.lib)")
    if start is not None and (resume is not None or capture_iteration is not None or reduce is not None or
                              coupling is not None or nccl_comm):
        raise ValueError("start cannot be combined with the state seam or a block-sharded solve")
    if factors is not False and factors is not None and (resume is not None or capture_iteration is not None):
        raise ValueError("factors cannot be combined with the state seam")
    o = options if options is not None else default_options()
    if trace_capacity:
        o.trace_capacity = int(trace_capacity)
    M = _Marshalled(prob, eig_resid, index_base)
    if reduce is not None:
        def _cb(ctx, ps, ns, pm, nm):
            try:
                sums = np.ctypeslib.as_array(ps, shape=(ns,)) if ns > 0 else np.zeros(0)
                maxs = np.ctypeslib.as_array(pm, shape=(nm,)) if nm > 0 else np.zeros(0)
                reduce(sums, maxs)
                return 0
            except Exception:                      # never unwind into C
                import traceback
                traceback.print_exc()
                return 1
        cb = REDUCE_FN(_cb)
        M.keep.append(cb)
        M.P.reduce_fn = C.cast(cb, C.c_void_p)
        M.P.reduce_ctx = None
    if nccl_comm:
        # native path: the library issues the collectives itself (RCCL, its own stream); no callbacks
        M.P.nccl_comm = C.c_void_p(int(nccl_comm))
    if coupling is not None and len(coupling["rows"]) > 0:
        rows = _i(coupling["rows"])                 # 0-based row numbers of [A;G], whatever index_base
        owned = np.ascontiguousarray(coupling["owned"], dtype=np.int32)
        M.keep += [rows, owned]
        M.P.n_coupling = len(rows)
        M.P.coupling_rows = _p(rows, pi64)
        M.P.coupling_owned = owned.ctypes.data_as(C.POINTER(i32))
        rv = coupling.get("reduce_vec")
        if rv is not None and not nccl_comm:
            def _cbv(ctx, ptr, length, on_device):
                try:
                    rv(int(ptr), int(length), bool(on_device))
                    return 0
                except Exception:
                    import traceback
                    traceback.print_exc()
                    return 1
            cbv = REDUCE_VEC_FN(_cbv)
            M.keep.append(cbv)
            M.P.reduce_vec_fn = C.cast(cbv, C.c_void_p)
            M.P.reduce_vec_on_device = 1 if coupling.get("on_device") else 0
    K = _SolveCall(int(M.P.n), int(M.P.p), int(M.P.m), psd_sides(prob), o, start, factors, primal, device_out)
    if on_device:
        return K.run(L.proxsdp_hip_solve_device, C.byref(M.P), C.byref(o), K.R, K.st, K.sd, K.F, K.out)
    if K.F is not None and K.st is None:
        return K.run(L.proxsdp_hip_solve_factored, C.byref(M.P), C.byref(o), K.R, K.F)
    if K.st is not None:
        return K.run(L.proxsdp_hip_solve_from, C.byref(M.P), C.byref(o), K.R, K.st, K.F)
    if resume is None and capture_iteration is None:
        return K.run(L.proxsdp_hip_solve, C.byref(M.P), C.byref(o), K.R)
    n, Q, nb = int(M.P.n), int(M.P.p + M.P.m), int(M.P.n_psd)
    rs = cs = carr = None
    if resume is not None:
        rs, rarr = _state_struct(n, Q, nb, o.convergence_window, state=resume)
    if capture_iteration is not None:
        cs, carr = _state_struct(n, Q, nb, o.convergence_window, iteration=capture_iteration)
    out = K.run(L.proxsdp_hip_solve_ex, C.byref(M.P), C.byref(o), K.R, _ref(rs), _ref(cs))
    out.state = _state_dict(cs, carr, n, Q, nb) if (cs is not None and cs.ints[3] == 1) else None
    return out


def _dump_arrays(D, fill):
    """the arrays of a proxsdp_model_dump whose sizes are known, allocated and bound (fill(D) is then called again)"""
    sizes = dict(n=int(D.n), Q=int(D.Q), nnz=int(D.nnz), ns=int(D.ns))
    arr = {}
    for name, sz in MODEL_DUMP_ARRAYS:
        a = np.zeros(max(sizes[sz], 1), dtype=np.int32 if name == "support" else np.float64)
        arr[name] = a
        setattr(D, name, a.ctypes.data_as(C.POINTER(i32)) if name == "support" else _p(a))
    fill(D)
    out = {name: arr[name][:sizes[sz]].copy() for name, sz in MODEL_DUMP_ARRAYS}
    out.update(sizes)
    out.update({k: float(D.norms[q]) for q, k in enumerate(MODEL_NORM_NAMES)})
    return out


def host_model_prepare(prob, index_base=0):
    """proxsdp_host_model_prepare: what a fresh Model of `prob` holds, computed on the host (no device), and the position maps:
    the dump's dictionary plus nnz_A, csc_pos, csr_pos (entry q of [A.data; G.data] in sorted CSC storage)."""
    L = lib()
    M = _Marshalled(prob, None, index_base)
    D = ModelDump()
    D.struct_size = C.sizeof(ModelDump)
    nnz_A = i64(0)
    _check(L.proxsdp_host_model_prepare(C.byref(M.P), C.byref(D), C.byref(nnz_A), None, None))
    cpos, rpos = np.zeros(max(int(D.nnz), 1), dtype=np.int32), np.zeros(max(int(D.nnz), 1), dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(i32))
    out = _dump_arrays(D, lambda d: _check(L.proxsdp_host_model_prepare(C.byref(M.P), C.byref(d), C.byref(nnz_A), ip(cpos), ip(rpos))))
    out.update(nnz_A=int(nnz_A.value), csc_pos=cpos[:out["nnz"]].copy(), csr_pos=rpos[:out["nnz"]].copy())
    return out


def _host_index(a):
    """an index array as a contiguous int64 NumPy array (a tensor, CUDA included, is copied to the host)"""
    if _is_tensor(a):
        a = a.detach().cpu().numpy()
    return _i(np.asarray(a).ravel())


def _rows_arguments(add, drop, n, index_base=0):
    """(drop, rowptr, cols, values, h_new) of a row change, the index arrays as int64 NumPy arrays (cols in `index_base`),
    values and h_new as given (NumPy or tensors); None where nothing is added / dropped.  add = (G_new, h_new) with G_new
    a scipy sparse k x n matrix or a triple (rowptr, cols, values) of CSR arrays with 0-based cols."""
    d = None if drop is None else _host_index(drop)
    if add is None:
        return d, None, None, None, None
    G_new, h_new = add
    if sp.issparse(G_new):
        G_new = sp.csr_matrix(G_new, dtype=np.float64)
        if G_new.shape[1] != n:
            raise ValueError(f"change_rows: the new rows must have {n} columns")
        ptr, cols, vals = G_new.indptr, G_new.indices, G_new.data
    else:
        ptr, cols, vals = G_new
    return d, _host_index(ptr), _host_index(cols) + index_base, vals, h_new


def _rows_struct(d, ptr, cols, vals, h_new, keep, R=None):
    """proxsdp_model_rows over HOST arrays (vals, h_new float64 NumPy, or None: R holds them already); keep collects what it
    points to"""
    R = ModelRows() if R is None else R
    R.struct_size = C.sizeof(ModelRows)
    if d is not None and len(d):
        keep.append(d)
        R.n_drop, R.drop = len(d), _p(d, pi64)
    if ptr is not None and len(ptr) > 1:
        keep += [ptr, cols if len(cols) else np.zeros(1, dtype=np.int64)]
        R.n_add, R.add_ptr, R.add_col = len(ptr) - 1, _p(ptr, pi64), _p(keep[-1], pi64)
        if vals is not None:
            keep += [vals if len(vals) else np.zeros(1), h_new]
            R.add_val, R.add_h = _p(keep[-2]), _p(keep[-1])
    return R


def host_model_rows_plan(prob, add=None, drop=None, index_base=0):
    """proxsdp_host_model_rows_plan: the planner Model.change_rows runs, on the host (no device).  prob: the model before
    the change.  Returns the dump's dictionary of the changed model plus csc_src, csr_src, bh_src (q >= 0: position q of
    the old array; -1 - t: entry t of the new values / right-hand sides), csc_pos, csr_pos, kept, m, nnz."""
    L = lib()
    M = _Marshalled(prob, None, index_base)
    d, ptr, cols, vals, h_new = _rows_arguments(add, drop, int(M.P.n), index_base)
    keep = []
    R = _rows_struct(d, ptr, cols, None if vals is None else _f(vals).ravel(), None if h_new is None else _f(h_new).ravel(), keep)
    kept = np.zeros(max(int(M.P.m) - int(R.n_drop) + int(R.n_add), 1), dtype=np.int64)
    R.kept = _p(kept, pi64)
    D = ModelDump()
    D.struct_size = C.sizeof(ModelDump)
    _check(L.proxsdp_host_model_rows_plan(C.byref(M.P), C.byref(R), C.byref(D), None, None, None, None, None))
    nz, Q = max(int(D.nnz), 1), max(int(D.Q), 1)
    maps = {k: np.zeros(Q if k == "bh_src" else nz, dtype=np.int32) for k in ("csc_src", "csr_src", "bh_src", "csc_pos", "csr_pos")}
    ip = lambda a: a.ctypes.data_as(C.POINTER(i32))
    out = _dump_arrays(D, lambda dd: _check(L.proxsdp_host_model_rows_plan(
        C.byref(M.P), C.byref(R), C.byref(dd), *[ip(maps[k]) for k in ("csc_src", "csr_src", "bh_src", "csc_pos", "csr_pos")])))
    out.update({k: v[:out["Q" if k == "bh_src" else "nnz"]].copy() for k, v in maps.items()})
    out.update(kept=kept[:int(R.m_new)].copy(), m=int(R.m_new))
    return out


class RowsChange:
    """What Model.change_rows did: kept (new inequality row r was old row kept[r], -1 for an added row), m, nnz,
    support_rebuilt, bytes_allocated, seconds."""

    def __init__(self, R, kept):
        self.kept = kept
        self.m, self.nnz = int(R.m_new), int(R.nnz_new)
        self.support_rebuilt = int(R.support_rebuilt)
        self.bytes_allocated, self.seconds = int(R.bytes_allocated), float(R.seconds)

    def carry(self, prev):
        """The start= dictionary of a previous result (or start dictionary) of the OLD shape for the changed model: dual_in
        re-indexed through `kept`, zeros on the new rows -- a NumPy array stays NumPy, a CUDA tensor stays on its device;
        everything else is passed through."""
        d = start_from_result(prev) if isinstance(prev, SolveResult) else dict(prev)
        v = d.get("dual_in")
        if v is None:
            return d
        old = np.maximum(self.kept, 0)
        if _is_tensor(v):
            import torch
            new = torch.zeros(len(self.kept), dtype=v.dtype, device=v.device)
            if len(self.kept) and v.numel():
                idx = torch.as_tensor(old, device=v.device)
                mask = torch.as_tensor(self.kept >= 0, device=v.device)
                new = torch.where(mask, v[idx], new)
        else:
            v = np.asarray(v, dtype=np.float64)
            new = np.zeros(len(self.kept))
            if len(self.kept) and len(v):
                new = np.where(self.kept >= 0, v[old], 0.0)
        d["dual_in"] = new
        return d


class TriangleCuts:
    """What a triangle separation returned (proxsdp_triangle_cuts): triples (rows x 3, 0-based i < j < k), patterns,
    violations (descending; equal ones by (i, j, k, pattern)), violated (all rows above min_violation), scanned, passes,
    seconds, sweep_seconds, bytes_allocated, and add = ((rowptr, cols, values), h) with 0-based cols: what
    Model.change_rows(add=...) and Optimizer.reoptimize(add_rows=...) take.  raw: add_col / add_val / add_h as the library
    wrote them (add_col in the index base of the model); arrays: every output array at its full length of `count` rows."""

    def __init__(self, T, arr, index_base):
        k = int(T.n_rows)
        self.arrays = arr
        self.triples = arr["tri"].reshape(-1, 3)[:k].copy()
        self.patterns = arr["pattern"][:k].copy()
        self.violations = arr["violation"][:k].copy()
        self.violated, self.scanned, self.passes = int(T.violated), int(T.scanned), int(T.passes)
        self.seconds, self.sweep_seconds = float(T.seconds), float(T.sweep_seconds)
        self.bytes_allocated = int(T.bytes_allocated)
        self.raw = dict(add_col=arr["add_col"][:3 * k].copy(), add_val=arr["add_val"][:3 * k].copy(), add_h=arr["add_h"][:k].copy())
        self.add = ((3 * np.arange(k + 1, dtype=np.int64), self.raw["add_col"] - index_base, self.raw["add_val"]),
                    self.raw["add_h"])

    def __len__(self):
        return len(self.patterns)


def _prefilled(arr, sentinel):
    """the output arrays of a tool call, every entry `sentinel` when one is given: what the library leaves alone shows"""
    if sentinel is not None:
        for a in arr.values():
            a[:] = sentinel
    return arr


def _dense_cone_arguments(who, X, cone_idx):
    """(X, idx) of a host separation: the square float64 matrix and the cone's variable list (None: the library's own)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != X.shape[1]:
        raise ValueError(f"{who}: X must be square")
    idx = None if cone_idx is None else _i(cone_idx)
    if idx is not None and len(idx) != X.shape[0] * (X.shape[0] + 1) // 2:
        raise ValueError(f"{who}: cone_idx must list the upper triangle")
    return X, idx


def _triangle_struct(count, min_violation, rhs, cand_cap, sentinel=None):
    """proxsdp_triangle_cuts with output arrays for `count` rows (prefilled with `sentinel` when given), and the arrays"""
    n = max(int(count), 1) if -(1 << 40) < int(count) < (1 << 24) else 1      # (an absurd count is the library's to refuse)
    arr = _prefilled(dict(tri=np.zeros(3 * n, dtype=np.int64), pattern=np.zeros(n, dtype=np.int32), violation=np.zeros(n),
                          add_col=np.zeros(3 * n, dtype=np.int64), add_val=np.zeros(3 * n), add_h=np.zeros(n)), sentinel)
    T = TriangleCutsIO()
    T.struct_size = C.sizeof(TriangleCutsIO)
    T.count, T.min_violation, T.rhs, T.cand_cap = int(count), float(min_violation), float(rhs), int(cand_cap)
    T.tri, T.add_col = _p(arr["tri"], pi64), _p(arr["add_col"], pi64)
    T.pattern = arr["pattern"].ctypes.data_as(C.POINTER(i32))
    T.violation, T.add_val, T.add_h = _p(arr["violation"]), _p(arr["add_val"]), _p(arr["add_h"])
    return T, arr


def host_triangle_cuts(X, count=1000, min_violation=1e-3, rhs=1.0, cone_idx=None, index_base=0, sentinel=None):
    """proxsdp_host_triangle_cuts: the separation of Model.separate_triangles on the host, serially (no device, no handle).
    X: the symmetric side x side matrix; cone_idx: the cone's variable list as add_col shall report it (None: tri_index +
    index_base).  Returns a TriangleCuts; its `arrays` are the output arrays at full length (entries past the rows returned
    keep `sentinel`)."""
    X, idx = _dense_cone_arguments("host_triangle_cuts", X, cone_idx)
    T, arr = _triangle_struct(count, min_violation, rhs, 0, sentinel)
    _check(lib().proxsdp_host_triangle_cuts(_p(X if X.size else np.zeros(1)), X.shape[0], None if idx is None else _p(idx, pi64),
                                            int(index_base), C.byref(T)))
    return TriangleCuts(T, arr, index_base)


TRIANGLE_PATTERN_SIGNS = np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1]], dtype=np.int8)


class CliqueCuts:
    """What a pentagonal / heptagonal separation returned (proxsdp_clique_cuts): nodes (rows x k, ascending, k = base size + 2),
    signs (rows x k int8, the first +1), violations (descending; equal ones by from_base), from_base (the base a row grew
    from; of merged bases the one with the greatest violation, then the lowest number), violated_bases (before merging),
    scanned, seconds, sweep_seconds, bytes_allocated, and add = ((rowptr, cols, values), h) with 0-based cols: what
    Model.change_rows(add=...) and Optimizer.reoptimize(add_rows=...) take.  raw: add_col / add_val / add_h as the library
    wrote them (add_col in the index base of the model); arrays: every output array at its full length of n_base rows, and the bases as they were passed.  A
    CliqueCuts of size 5 is itself a set of bases for the next call."""

    def __init__(self, Q, arr, index_base):
        n, k = int(Q.n_rows), int(Q.base_size) + 2
        npair = k * (k - 1) // 2
        self.arrays = arr
        self.size = k
        self.nodes = arr["nodes"].reshape(-1, k)[:n].copy()
        self.signs = arr["signs"].reshape(-1, k)[:n].copy()
        self.violations = arr["violation"][:n].copy()
        self.from_base = arr["from_base"][:n].copy()
        self.violated_bases, self.scanned = int(Q.violated_bases), int(Q.scanned)
        self.seconds, self.sweep_seconds = float(Q.seconds), float(Q.sweep_seconds)
        self.bytes_allocated = int(Q.bytes_allocated)
        self.raw = dict(add_col=arr["add_col"][:npair * n].copy(), add_val=arr["add_val"][:npair * n].copy(),
                        add_h=arr["add_h"][:n].copy())
        self.add = ((npair * np.arange(n + 1, dtype=np.int64), self.raw["add_col"] - index_base, self.raw["add_val"]),
                    self.raw["add_h"])

    def __len__(self):
        return len(self.violations)


def _clique_bases(bases):
    """(nodes, signs) as contiguous n_base x q int64 / int8 arrays from a TriangleCuts (patterns 0: (+,+,+), 1: (+,+,-),
    2: (+,-,+), 3: (+,-,-): the triangle rows' own signs in the normal form of a base), a CliqueCuts or a pair"""
    if isinstance(bases, TriangleCuts):
        nodes, signs = bases.triples, TRIANGLE_PATTERN_SIGNS[bases.patterns]
    elif isinstance(bases, CliqueCuts):
        nodes, signs = bases.nodes, bases.signs
    else:
        nodes, signs = bases
    nodes = np.ascontiguousarray(nodes, dtype=np.int64)
    signs = np.ascontiguousarray(signs, dtype=np.int8)
    if nodes.ndim != 2 or nodes.shape != signs.shape:
        raise ValueError("separate_cliques: bases must be n_base x q nodes and as many signs")
    return nodes, signs


def _clique_struct(nodes, signs, min_violation, rhs, knobs=None, sentinel=None):
    """proxsdp_clique_cuts for those bases with output arrays for n_base rows (prefilled with `sentinel` when given), and the
    arrays.  rhs None: (q + 1) / 2.  knobs: {grid: workgroup columns of the sweep, batch: bases per launch}"""
    nb, q = nodes.shape
    n, k = max(nb, 1), q + 2
    npair = k * (k - 1) // 2
    arr = _prefilled(dict(nodes=np.zeros(k * n, dtype=np.int64), signs=np.zeros(k * n, dtype=np.int8), violation=np.zeros(n),
                          from_base=np.zeros(n, dtype=np.int64), add_col=np.zeros(npair * n, dtype=np.int64),
                          add_val=np.zeros(npair * n), add_h=np.zeros(n)), sentinel)
    Q = CliqueCutsIO()
    Q.struct_size = C.sizeof(CliqueCutsIO)
    Q.base_size, Q.n_base = int(q), int(nb)
    Q.rhs = float((q + 1) / 2 if rhs is None else rhs)
    Q.min_violation = float(min_violation)
    for name, v in dict(knobs or {}).items():
        if name not in ("grid", "batch"):
            raise ValueError(f"separate_cliques: no knob {name}")
        setattr(Q, name, int(v))
    # (the bases travel with the output arrays, so that they live as long as the struct points at them; no base: any
    # non-NULL address, n_base = 0 is the library's to refuse)
    arr["base_nodes"] = nodes if nodes.size else np.zeros(1, dtype=np.int64)
    arr["base_sign"] = signs if signs.size else np.zeros(1, dtype=np.int8)
    Q.base_nodes = _p(arr["base_nodes"], pi64)
    Q.base_sign = arr["base_sign"].ctypes.data_as(C.POINTER(C.c_int8))
    Q.nodes, Q.from_base, Q.add_col = _p(arr["nodes"], pi64), _p(arr["from_base"], pi64), _p(arr["add_col"], pi64)
    Q.signs = arr["signs"].ctypes.data_as(C.POINTER(C.c_int8))
    Q.violation, Q.add_val, Q.add_h = _p(arr["violation"]), _p(arr["add_val"]), _p(arr["add_h"])
    return Q, arr


def host_clique_cuts(X, bases, min_violation=1e-3, rhs=None, cone_idx=None, index_base=0, sentinel=None):
    """proxsdp_host_clique_cuts: the separation of Model.separate_cliques on the host, serially (no device, no handle).  X: the
    symmetric side x side matrix; bases: as Model.separate_cliques takes them; cone_idx: the cone's variable list as add_col
    shall report it (None: tri_index + index_base).  Returns a CliqueCuts; its `arrays` are the output arrays at full length
    (entries past the rows returned keep `sentinel`)."""
    X, idx = _dense_cone_arguments("host_clique_cuts", X, cone_idx)
    nodes, signs = _clique_bases(bases)
    Q, arr = _clique_struct(nodes, signs, min_violation, rhs, None, sentinel)
    _check(lib().proxsdp_host_clique_cuts(_p(X if X.size else np.zeros(1)), X.shape[0], None if idx is None else _p(idx, pi64),
                                          int(index_base), C.byref(Q)))
    return CliqueCuts(Q, arr, index_base)


class Rounding:
    """What a rounding returned (proxsdp_rounding): signs (int8, +-1, one per node of the cone), value (of `signs`, the
    cone's part of c'x in the units and the minimisation form of the model's c), value_rounded (the smallest value before the
    local search), best_trial, sweeps, flips, values_rounded / values_final (one per trial), seconds, search_seconds,
    bytes_allocated, and adjacency = (ptr, cols, values, diag) as the library derived it from c, when asked for (else None).
    objective: set by Optimizer.round.  arrays: every output array at its full length."""

    def __init__(self, Q, arr):
        self.arrays = arr
        self.signs = arr["signs"].copy()
        self.value, self.value_rounded = float(Q.value), float(Q.value_rounded)
        self.best_trial, self.sweeps, self.flips = int(Q.best_trial), int(Q.sweeps), int(Q.flips)
        self.values_rounded, self.values_final = arr["values_rounded"].copy(), arr["values_final"].copy()
        self.seconds, self.search_seconds = float(Q.seconds), float(Q.search_seconds)
        self.bytes_allocated = int(Q.bytes_allocated)
        self.adjacency = None
        if "adj_ptr" in arr:
            k = int(Q.adj_nnz)
            self.adjacency = (arr["adj_ptr"].copy(), arr["adj_col"][:k].copy(), arr["adj_val"][:k].copy(), arr["diag"].copy())
        self.objective = None


def _rounding_struct(side, r, trials, seed, max_sweeps, knobs=None, adj_cap=None, sentinel=None):
    """proxsdp_rounding with output arrays for a cone of that side (prefilled with `sentinel` when given), and the arrays.
    knobs: {grid_adjacency, grid_directions, grid_signs, grid_search: workgroups; lds_side: None = the library's choice, 0 =
    never in LDS}; adj_cap: room for the adjacency (None: not asked for)"""
    s = max(int(side), 1)
    nt = int(trials) if 0 < int(trials) <= (1 << 20) else 1         # (an absurd count is the library's to refuse)
    arr = dict(signs=np.zeros(s, dtype=np.int8), values_rounded=np.zeros(nt), values_final=np.zeros(nt))
    if adj_cap is not None:
        cap = max(int(adj_cap), 1)
        arr.update(adj_ptr=np.zeros(s + 1, dtype=np.int64), adj_col=np.zeros(cap, dtype=np.int64), adj_val=np.zeros(cap),
                   diag=np.zeros(s))
    _prefilled(arr, sentinel)
    Q = RoundingIO()
    Q.struct_size = C.sizeof(RoundingIO)
    Q.r, Q.trials, Q.seed, Q.max_sweeps = int(r), int(trials), int(seed), int(max_sweeps)
    knobs = dict(knobs or {})
    lds = knobs.pop("lds_side", None)
    Q.lds_side = 0 if lds is None else (-1 if int(lds) <= 0 else int(lds))
    for k, v in knobs.items():
        if k not in ("grid_adjacency", "grid_directions", "grid_signs", "grid_search"):
            raise ValueError(f"round: no knob {k}")
        setattr(Q, k, int(v))
    Q.signs = arr["signs"].ctypes.data_as(C.POINTER(C.c_int8))
    Q.values_rounded, Q.values_final = _p(arr["values_rounded"]), _p(arr["values_final"])
    if adj_cap is not None:
        Q.adj_ptr, Q.adj_col, Q.adj_val, Q.diag = _p(arr["adj_ptr"], pi64), _p(arr["adj_col"], pi64), _p(arr["adj_val"]), _p(arr["diag"])
        Q.adj_cap = int(adj_cap)
    return Q, arr


def host_round_directions(seed, r, trials):
    """proxsdp_host_round_directions: the r x trials directions g(k, t) of a rounding with that seed"""
    g = np.zeros((max(int(r), 1), int(trials) if 0 < int(trials) <= (1 << 20) else 1))
    _check(lib().proxsdp_host_round_directions(int(seed), int(r), int(trials), _p(g)))
    return g


def host_round(values, vectors, adjacency, trials=1024, seed=0, max_sweeps=50, sentinel=None):
    """proxsdp_host_round: the rounding of Model.round on the host, serially (no device, no handle).  values (r,) and
    vectors (side, r): the factors; adjacency = (ptr, cols, values, diag) of the objective.  Returns a Rounding."""
    vals = _f(values).ravel()
    V = np.asarray(vectors, dtype=np.float64)
    if V.ndim != 2 or V.shape[1] != len(vals):
        raise ValueError("host_round: vectors must be side x len(values)")
    side = V.shape[0]
    Vf = np.ascontiguousarray(V.T).ravel()                          # column-major, ld = side
    ptr, cols, av, diag = adjacency
    ptr, cols, av, diag = _i(ptr), _i(cols), _f(av), _f(diag)
    if len(ptr) != side + 1 or len(diag) != side or len(cols) != len(av) or (len(ptr) and len(cols) < ptr[-1]):
        raise ValueError("host_round: the adjacency does not fit the side")
    Q, arr = _rounding_struct(side, len(vals), trials, seed, max_sweeps, sentinel=sentinel)
    Q.V, Q.values = _p(Vf if Vf.size else np.zeros(1)), _p(vals if vals.size else np.zeros(1))
    _check(lib().proxsdp_host_round(side, _p(ptr, pi64), _p(cols if len(cols) else np.zeros(1, dtype=np.int64), pi64),
                                    _p(av if len(av) else np.zeros(1)), _p(diag if len(diag) else np.zeros(1)), C.byref(Q)))
    return Rounding(Q, arr)


class DualBound:
    """What a bound call returned (proxsdp_dual_bound): bound (a certified LOWER bound of min c'x in the units and the
    minimisation form of the model's c; -inf when some cone could not be certified), dual_objective (d), and per PSD cone
    shift (sigma*), lambda_lower (l_k), radius (rho_k), delta, trace (T_k), factorisations, certified; loss = sum_k
    T_k (shift + delta + radius), what the certificate costs beside the ideal bound of the same duals; seconds,
    factor_seconds, bytes_allocated.  objective: set by Optimizer.bound (the bound in the model's own sense)."""

    def __init__(self, Q, arr):
        self.arrays = arr
        self.bound, self.dual_objective = float(Q.bound), float(Q.dual_objective)
        for k in ("shift", "lambda_lower", "radius", "delta", "factorisations", "certified"):
            setattr(self, k, arr[k].copy())
        self.trace = arr["trace_used"].copy()
        self.certified = self.certified.astype(bool)
        with np.errstate(invalid="ignore"):
            self.loss = float(np.sum(self.trace * (self.shift + self.delta + self.radius)))
        self.seconds, self.factor_seconds = float(Q.seconds), float(Q.factor_seconds)
        self.bytes_allocated = int(Q.bytes_allocated)
        self.objective = None


def _bound_struct(n_psd, trace_cap=None, sentinel=None):
    """proxsdp_dual_bound with output arrays for n_psd cones (prefilled with `sentinel` when given), and the arrays"""
    k = max(int(n_psd), 1)
    arr = _prefilled(dict(shift=np.zeros(k), lambda_lower=np.zeros(k), radius=np.zeros(k), delta=np.zeros(k), trace_used=np.zeros(k),
                          factorisations=np.zeros(k, dtype=np.int32), certified=np.zeros(k, dtype=np.int32)), sentinel)
    Q = DualBoundIO()
    Q.struct_size = C.sizeof(DualBoundIO)
    for name in ("shift", "lambda_lower", "radius", "delta", "trace_used"):
        setattr(Q, name, _p(arr[name]))
    Q.factorisations, Q.certified = _p(arr["factorisations"], C.POINTER(i32)), _p(arr["certified"], C.POINTER(i32))
    if trace_cap is not None:
        cap = _f(trace_cap).ravel()
        if len(cap) != int(n_psd):
            raise ValueError(f"bound: trace_cap must have {n_psd} entries, one per PSD cone")
        arr["trace_cap"] = cap
        Q.trace_cap = _p(cap if len(cap) else np.zeros(1))
    return Q, arr


def host_dual_bound(prob, dual_eq, dual_in, trace_cap=None, index_base=0, sentinel=None):
    """proxsdp_host_dual_bound: the certified bound of Model.bound on the host, serially (no device, no handle).  prob: a
    problem (c, A, b, G, h, psd); dual_eq (p) and dual_in (m): any dual point.  Returns a DualBound."""
    A, G = sp.csc_matrix(prob.A, dtype=np.float64), sp.csc_matrix(prob.G, dtype=np.float64)
    p, m, n = A.shape[0], G.shape[0], int(prob.n)
    M = sp.vstack([A, G], format="csc") if p + m else sp.csc_matrix((0, n))
    M.sort_indices()
    cp, rv, nz = _i(M.indptr) + index_base, _i(M.indices) + index_base, _f(M.data)
    Mc = CSC(p + m, n, _p(cp, pi64), _p(rv if len(rv) else np.zeros(1, dtype=np.int64), pi64), _p(nz if len(nz) else np.zeros(1)))
    bh = _f(np.concatenate([np.asarray(prob.b, float).ravel(), np.asarray(prob.h, float).ravel()]))
    c = _f(prob.c).ravel()
    lst = list(prob.psd)
    ptr = np.zeros(len(lst) + 1, dtype=np.int64)
    for k, v in enumerate(lst):
        ptr[k + 1] = ptr[k] + len(v)
    idx = (_i(np.concatenate(lst)) + index_base) if lst else np.zeros(1, dtype=np.int64)
    ye, yi = _f(dual_eq).ravel(), _f(dual_in).ravel()
    if len(ye) != p or len(yi) != m:
        raise ValueError(f"host_dual_bound: dual_eq and dual_in must have {p} and {m} entries")
    Q, arr = _bound_struct(len(lst), trace_cap, sentinel)
    Q.dual_eq, Q.dual_in = _p(ye if p else np.zeros(1)), _p(yi if m else np.zeros(1))
    _check(lib().proxsdp_host_dual_bound(n, p, m, _p(c if n else np.zeros(1)), C.byref(Mc), _p(bh if len(bh) else np.zeros(1)),
                                         len(lst), _p(ptr, pi64), _p(idx, pi64), index_base, C.byref(Q)))
    return DualBound(Q, arr)


def _cholesky(entry, A, shift, want_factor):
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("cholesky: A must be square")
    s = A.shape[0]
    R = np.zeros((s, s)) if want_factor else None
    fail = C.c_int64(-2)
    _check(entry(_p(A if s else np.zeros(1)), s, float(shift), _p(R) if want_factor else None, C.byref(fail)))
    return int(fail.value), R


def cholesky(A, shift=0.0, want_factor=True):
    """proxsdp_hip_cholesky: ONE factorisation of A + shift I by the device kernels of Model.bound (test entry).  Returns
    (fail_col, R): fail_col = -1 when it completed, else the first failing column; R upper triangular, R'R ~ A + shift I."""
    return _cholesky(lib().proxsdp_hip_cholesky, A, shift, want_factor)


def host_cholesky(A, shift=0.0, want_factor=True):
    """proxsdp_host_cholesky: the same by the plain serial column Cholesky of the host half (no device)"""
    return _cholesky(lib().proxsdp_host_cholesky, A, shift, want_factor)


def model_norm2(v, grid=0):
    """proxsdp_hip_model_norm2: ||v||_2 by the reduction a device-route Model.update uses, with `grid` workgroups"""
    v = _f(v).ravel()
    out = f64()
    _check(lib().proxsdp_hip_model_norm2(_p(v if len(v) else np.zeros(1)), len(v), int(grid), C.byref(out)))
    return out.value


class Model:
    """A model that stays set up on the device between solves (proxsdp_hip_model_*, include/proxsdp_hip.h).

        with Model(prob, options) as mdl:
            r0 = mdl.solve(factors=True, device_out=True)
            mdl.update(c=new_c)                      # same shape, new numbers
            r1 = mdl.solve(start=r0, factors=True, device_out=True)

    The set-up of solve() -- validation, ordering, scaling, the operator, the workspaces -- runs once, in the constructor;
    solve() is solve(prob, options, ..., device_out=...) on the model's current data bit for bit (only the clocks differ).
    The ctypes problem is built once, here; nothing of `prob` is referenced afterwards."""

    def __init__(self, prob, options=None, eig_resid=None, index_base=0):
        L = lib()
        o = options if options is not None else default_options()
        self._options = Options.from_buffer_copy(o)
        M = _Marshalled(prob, eig_resid, index_base)
        self.n, self.p, self.m = int(M.P.n), int(M.P.p), int(M.P.m)
        self._sides = psd_sides(prob)
        self._nnz = (int(sp.csc_matrix(prob.A).nnz), int(sp.csc_matrix(prob.G).nnz))
        self._index_base = index_base
        self._h = C.c_void_p()
        _check(L.proxsdp_hip_model_create(C.byref(M.P), C.byref(self._options), C.byref(self._h)))

    # ---- lifetime
    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _check(lib().proxsdp_hip_model_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise ValueError("the model is closed")
        return self._h

    def _route(self, who, S, fields, short=None):
        """The host-or-device marshalling of a call.  fields: {field of the struct S: (value, entries, label)}, each value a
        NumPy array (a CPU tensor counts as one) or a CUDA float64 tensor.  All CUDA tensors: the device route -- S.on_device
        = 1, the tensors' own addresses, one synchronize (the library runs on its own stream).  Otherwise the host route:
        contiguous float64 arrays, one zero in place of an empty one (any non-NULL address).  A mixture is a ValueError, and
        so is a wrong length (`short`: the text of that refusal where the call names its fields together).  Returns
        (on_device, keep); keep holds what S points to and has to outlive the call."""
        on_dev = [_is_tensor(v) and v.is_cuda for v, _, _ in fields.values()]
        if any(on_dev) and not all(on_dev):
            raise ValueError(f"{who}: host arrays and CUDA tensors cannot be mixed in one call")
        if fields and all(on_dev):
            import torch
            dev_id = int(self._options.device_id)
            S.on_device = 1
            for k, (v, ln, what) in fields.items():
                setattr(S, k, _device_ptr(v, ln, dev_id, what))
            torch.cuda.synchronize(dev_id)
            return True, [v for v, _, _ in fields.values()]
        keep = []
        for k, (v, ln, what) in fields.items():
            a = _f(v.numpy() if _is_tensor(v) else v).ravel()
            if len(a) != ln:
                raise ValueError(f"{who}: " + (short or f"{what} must have {ln} entries"))
            keep.append(a if len(a) else np.zeros(1))
            setattr(S, k, _p(keep[-1]))
        return False, keep

    # ---- data
    def update(self, c=None, b=None, h=None, A_values=None, G_values=None):
        """Replace data of the same shape: c (n), b (p), h (m) in the caller's order; A_values / G_values = the stored entries
        of A / G in sorted CSC order (scipy's .data after sort_indices), or a sparse matrix with the pattern the model was
        built with.  NumPy arrays go the host route, CUDA float64 tensors the device route (proxsdp_model_data.on_device);
        mixing the two in one call is a ValueError."""
        fields = {}
        for k, v, ln in (("c", c, self.n), ("b", b, self.p), ("h", h, self.m), ("A_nzval", A_values, self._nnz[0]),
                         ("G_nzval", G_values, self._nnz[1])):
            if sp.issparse(v):
                v = sp.csc_matrix(v, dtype=np.float64)
                v.sort_indices()
                v = v.data
            if v is not None:
                fields[k] = (v, ln, k)
        D = ModelData()
        D.struct_size = C.sizeof(ModelData)
        _, keep = self._route("Model.update", D, fields)
        _check(lib().proxsdp_hip_model_update(self._handle(), C.byref(D)))
        del keep

    def change_rows(self, add=None, drop=None):
        """proxsdp_hip_model_rows: add and drop inequality rows in place.  drop: numbers (0-based) into the model's current
        G.  add = (G_new, h_new): G_new a scipy sparse k x n matrix or a triple (rowptr, cols, values) of CSR arrays
        (0-based cols), h_new the k right-hand sides.  G' = [kept rows in their old order; the new rows], stored column by
        column: kept entries first, then the new ones by ascending row -- the order a later update(G_values=...) follows.
        values / h_new as CUDA float64 tensors take the device route, NumPy arrays the host route; mixing the two is a
        ValueError.  Index arrays that arrive as tensors are copied to the host.  Returns a RowsChange; carry(prev) of it
        re-indexes a previous result's dual_in for start=."""
        d, ptr, cols, vals, h_new = _rows_arguments(add, drop, self.n)
        fields = {}
        if ptr is not None:
            fields = dict(add_val=(vals, int(ptr[-1]), "values"), add_h=(h_new, len(ptr) - 1, "h_new"))
        R = ModelRows()                                      # (the values first: what they are refused for needs no index array)
        _, keep = self._route("Model.change_rows", R, fields)
        _rows_struct(d, ptr, None if cols is None else cols + self._index_base, None, None, keep, R)
        kept = np.zeros(max(self.m - int(R.n_drop) + int(R.n_add), 1), dtype=np.int64)
        R.kept = _p(kept, pi64)
        _check(lib().proxsdp_hip_model_rows(self._handle(), C.byref(R)))
        del keep
        self.m = int(R.m_new)
        self._nnz = (self._nnz[0], int(R.nnz_new) - self._nnz[0])
        return RowsChange(R, kept[:self.m].copy())

    # ---- separation
    def separate_triangles(self, primal, cone=0, count=1000, min_violation=1e-3, rhs=1.0, cand_cap=0):
        """proxsdp_hip_model_triangles: the `count` most violated triangle inequalities of PSD cone `cone` at `primal` -- a
        NumPy array (host route), a CUDA float64 tensor (device route) or a SolveResult (its primal) of n entries.  Returns a
        TriangleCuts; change_rows(add=cuts.add) appends the rows.  The model is not touched."""
        if isinstance(primal, SolveResult):
            primal = primal.primal
        if primal is None:
            raise ValueError("Model.separate_triangles: the result holds no primal (solve(primal=True))")
        T, arr = _triangle_struct(count, min_violation, rhs, cand_cap)
        T.cone = int(cone)
        _, keep = self._route("Model.separate_triangles", T, dict(primal=(primal, self.n, "primal")))
        _check(lib().proxsdp_hip_model_triangles(self._handle(), C.byref(T)))
        del keep
        return TriangleCuts(T, arr, self._index_base)

    def separate_cliques(self, primal, bases, cone=0, min_violation=1e-3, rhs=None, knobs=None):
        """proxsdp_hip_model_cliques: every base grown by its most violated pair of further nodes and signs of PSD cone `cone`
        at `primal` (as separate_triangles takes it) -- pentagonal rows from triangles, heptagonal rows from pentagons.  bases:
        a TriangleCuts, a CliqueCuts of size 5, or (nodes, signs) as n_base x q arrays (q = 3 or 5; nodes 0-based and ascending,
        signs +-1 with the first +1).  rhs None: (q + 1) / 2.  knobs: test knobs (_clique_struct).  Returns a CliqueCuts;
        change_rows(add=cuts.add) appends the rows.  The model is not touched."""
        if isinstance(primal, SolveResult):
            primal = primal.primal
        if primal is None:
            raise ValueError("Model.separate_cliques: the result holds no primal (solve(primal=True))")
        nodes, signs = _clique_bases(bases)
        Q, arr = _clique_struct(nodes, signs, min_violation, rhs, knobs)
        Q.cone = int(cone)
        _, keep = self._route("Model.separate_cliques", Q, dict(primal=(primal, self.n, "primal")))
        _check(lib().proxsdp_hip_model_cliques(self._handle(), C.byref(Q)))
        del keep
        return CliqueCuts(Q, arr, self._index_base)

    def inactive_rows(self, result_or_pair, dual_tol=0.0, slack_tol=1e-6):
        """proxsdp_hip_model_inactive_rows: the inequality rows r with |dual_in[r]| <= dual_tol and slack_in[r] < -slack_tol
        (slack_in = G x - h) as an ascending int64 array of 0-based numbers -- a drop list for change_rows.  result_or_pair: a
        SolveResult or (dual_in, slack_in), both NumPy or both CUDA float64 tensors.  A NaN row is not inactive."""
        if isinstance(result_or_pair, SolveResult):
            dual, slack = result_or_pair.dual_in, result_or_pair.slack_in
        else:
            dual, slack = result_or_pair
        Q = InactiveRowsIO()
        Q.struct_size = C.sizeof(InactiveRowsIO)
        Q.dual_tol, Q.slack_tol = float(dual_tol), float(slack_tol)
        rows = np.zeros(max(self.m, 1), dtype=np.int64)
        Q.rows = _p(rows, pi64)
        on_dev, keep = self._route("Model.inactive_rows", Q, dict(dual_in=(dual, self.m, "dual_in"), slack_in=(slack, self.m, "slack_in")),
                                   short=f"dual_in and slack_in must have {self.m} entries")
        if on_dev and not self.m:                            # (no row: any non-NULL address, never read)
            keep.append(np.zeros(1))
            Q.dual_in = Q.slack_in = _p(keep[-1])
        _check(lib().proxsdp_hip_model_inactive_rows(self._handle(), C.byref(Q)))
        del keep
        return rows[:int(Q.n_rows)].copy()

    # ---- a feasible point
    def round(self, factors, cone=0, trials=1024, seed=0, max_sweeps=50, adjacency=False, knobs=None):
        """proxsdp_hip_model_round: randomised hyperplane rounding of the factors of PSD cone `cone` to `trials` +-1 vectors
        and a one-flip local search against the model's current c, on the device; the best vector and its value.  factors:
        (values, vectors) as NumPy arrays (host route) or as CUDA float64 tensors (device route; mixing the two is a
        ValueError), vectors of shape (side, r) -- or a SolveResult that carries factors (solve(factors=...)).
        adjacency=True also returns the objective's adjacency as the library derived it; knobs: test knobs
        (_rounding_struct).  Returns a Rounding.  The model is not touched."""
        if isinstance(factors, SolveResult):
            fl = getattr(factors, "psd_factors", None)
            if fl is None:
                raise ValueError("Model.round: the result carries no factors (solve(factors=True))")
            factors = fl[cone][:2]
        vals, V = factors[0], factors[1]
        side = self._sides[cone] if 0 <= int(cone) < len(self._sides) else 1
        if len(V.shape) != 2 or V.shape[1] != len(vals) or (0 <= int(cone) < len(self._sides) and V.shape[0] != side):
            raise ValueError(f"Model.round: vectors must be side x len(values) = {side} x {len(vals)}")
        Q, arr = _rounding_struct(side, len(vals), trials, seed, max_sweeps, knobs, side * (side - 1) if adjacency else None)
        Q.cone = int(cone)
        Vt = V.t().contiguous() if _is_tensor(V) else np.asarray(V, dtype=np.float64).T     # column-major, ld = side
        _, keep = self._route("Model.round", Q, dict(V=(Vt, V.shape[0] * V.shape[1], "vectors"), values=(vals, len(vals), "values")))
        _check(lib().proxsdp_hip_model_round(self._handle(), C.byref(Q)))
        del keep
        return Rounding(Q, arr)

    # ---- a bound
    def bound(self, duals, trace_cap=None):
        """proxsdp_hip_model_bound: a certified LOWER bound of the model's optimum (minimisation form) from any dual point --
        the proof is a completed fp64 Cholesky factorisation on the device with its backward-error bound, no eigenvalue
        estimate.  duals: a SolveResult or (dual_eq, dual_in), both NumPy or both CUDA float64 tensors.  trace_cap: one number
        per PSD cone with tr X_k <= cap for every feasible x, or None = derived from equality rows a X_ii = b.  Returns a
        DualBound.  The model is not touched."""
        if isinstance(duals, SolveResult):
            duals = (duals.dual_eq, duals.dual_in)
        ye, yi = duals
        Q, arr = _bound_struct(len(self._sides), trace_cap)
        fields = dict(dual_eq=(ye, self.p, "dual_eq"), dual_in=(yi, self.m, "dual_in"))
        on_dev, keep = self._route("Model.bound", Q, fields, short=f"dual_eq and dual_in must have {self.p} and {self.m} entries")
        for k, (_, ln, _) in fields.items():
            if on_dev and not ln:                            # (no row: any non-NULL address, never read)
                keep.append(np.zeros(1))
                setattr(Q, k, _p(keep[-1]))
        _check(lib().proxsdp_hip_model_bound(self._handle(), C.byref(Q)))
        del keep
        return DualBound(Q, arr)

    # ---- solve
    def solve(self, start=None, factors=False, primal=True, device_out=False, trace_capacity=0, time_limit=None,
              max_iter=None):
        """proxsdp_hip_model_solve: the SolveResult solve(prob, options, start=..., factors=..., primal=..., device_out=...)
        returns for the model's current data.  trace_capacity, time_limit and max_iter override the model's options for this
        solve (they shape nothing in the set-up)."""
        L = lib()
        o = Options.from_buffer_copy(self._options)
        if trace_capacity:
            o.trace_capacity = int(trace_capacity)
        if time_limit is not None:
            o.time_limit = float(time_limit)
        if max_iter is not None:
            o.max_iter = int(max_iter)
        K = _SolveCall(self.n, self.p, self.m, self._sides, o, start, factors, primal, device_out)
        return K.run(L.proxsdp_hip_model_solve, self._handle(), C.byref(o), K.R, K.st, K.sd, K.F, K.out)

    # ---- what it holds
    def info(self):
        I = ModelInfo()
        I.struct_size = C.sizeof(ModelInfo)
        _check(lib().proxsdp_hip_model_info(self._handle(), C.byref(I)))
        return {k: getattr(I, k) for k, _ in ModelInfo._fields_ if k != "struct_size"}

    def dump(self):
        """proxsdp_hip_model_dump: the model's internal data as a dictionary (test entry)"""
        L = lib()
        D = ModelDump()
        D.struct_size = C.sizeof(ModelDump)
        _check(L.proxsdp_hip_model_dump(self._handle(), C.byref(D)))
        return _dump_arrays(D, lambda d: _check(L.proxsdp_hip_model_dump(self._handle(), C.byref(d))))


def exit_vectors(prob, x, y, zero_c=False, options=None, index_base=0):
    """proxsdp_hip_exit_vectors: the device exit path alone on a host iterate (x: n, solver order and scale as the loop leaves
    it; y: p + m).  Returns dict(primal, dual_cone, dual_eq, dual_in, slack_eq, slack_in, viol (4: inequality duals, 1x1 cones,
    second-order cones, free variables), neg (minus the dual-cone block of every PSD cone of side >= 2, in cone order))."""
    L = lib()
    o = options if options is not None else default_options()
    M = _Marshalled(prob, None, index_base)
    n, p, m = int(M.P.n), int(M.P.p), int(M.P.m)
    x, y = _f(x).ravel(), _f(y).ravel()
    if len(x) != n or len(y) != p + m:
        raise ValueError("exit_vectors: x must have n entries and y p + m")
    lens = dict(primal=n, dual_cone=n, dual_eq=p, dual_in=m, slack_eq=p, slack_in=m)
    out = {k: np.full(max(v, 1), np.nan) for k, v in lens.items()}
    nneg = sum(len(v) for v, sd in zip(prob.psd, psd_sides(prob)) if sd >= 2)
    viol, neg = np.full(4, np.nan), np.full(max(nneg, 1), np.nan)
    xs, ys = (x if n else np.zeros(1)), (y if p + m else np.zeros(1))
    _check(L.proxsdp_hip_exit_vectors(C.byref(M.P), C.byref(o), _p(xs), _p(ys), 1 if zero_c else 0,
                                      *[_p(out[k]) for k in ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in")],
                                      _p(viol), _p(neg), nneg))
    d = {k: out[k][:v] for k, v in lens.items()}
    d.update(viol=viol, neg=neg[:nneg])
    return d


def _owner_arrays(owners, soc_owners, free_owners):
    """int32 arrays (kept alive by the caller) and their pointers; None -> NULL = the library's round-robin default"""
    arrs = [None if o is None else np.ascontiguousarray(o, dtype=np.int32) for o in (owners, soc_owners, free_owners)]
    # (an empty list is a valid owner list of a model without such cones: hand over a pointer, not NULL)
    arrs = [a if (a is None or len(a)) else np.zeros(1, dtype=np.int32) for a in arrs]
    return arrs, [None if a is None else _p(a, C.POINTER(i32)) for a in arrs]


def solve_sharded_inprocess(prob, n_shards, device_ids=None, owners=None, soc_owners=None, free_owners=None, options=None,
                            trace_capacity=0, eig_resid=None, index_base=0):
    """proxsdp_hip_solve_sharded: the WHOLE model in, split by the library into n_shards shards that run as host threads of
    this process (shard s on device_ids[s]; default: all on options.device_id), the whole model's result out, in the
    caller's order.  owners / soc_owners / free_owners: shard per PSD cone / SOC cone / free variable (None = one
    round-robin, sharded.default_owners).  Returns (SolveResult, [per-shard stats dicts])."""
    L = lib()
    o = options if options is not None else default_options()
    if trace_capacity:
        o.trace_capacity = int(trace_capacity)
    n_shards = int(n_shards)
    M = _Marshalled(prob, eig_resid, index_base)
    keep, ptrs = _owner_arrays(owners, soc_owners, free_owners)
    dev = None
    if device_ids is not None:
        dev = np.ascontiguousarray(device_ids, dtype=np.int32)
        if len(dev) != n_shards:
            raise ValueError("device_ids: one device per shard")
    n, p, m = M.P.n, M.P.p, M.P.m
    arrays = [np.zeros(max(k, 1)) for k in (n, n, p, m, p, m)]
    trace = np.zeros((max(o.trace_capacity, 1), TRACE_COLS))
    R = Result()
    R.primal, R.dual_cone, R.dual_eq, R.dual_in, R.slack_eq, R.slack_in = [_p(a) for a in arrays]
    R.trace = _p(trace)
    SS = (Stats * max(n_shards, 1))()
    _check(L.proxsdp_hip_solve_sharded(C.byref(M.P), C.byref(o), n_shards, _p(dev, C.POINTER(i32)) if dev is not None else None,
                                       ptrs[0], ptrs[1], ptrs[2], C.byref(R), SS))
    del keep
    arrays = [a[:k] for a, k in zip(arrays, (n, n, p, m, p, m))]
    sol = SolveResult(R, n, p, m, arrays, trace)
    shard_stats = []
    for s in range(n_shards):
        d = {k: (list(getattr(SS[s], k)) if k.startswith("reserved") else getattr(SS[s], k)) for k, _ in Stats._fields_}
        for k, slot in STATS_RESERVED_SLOTS.items():
            d[k] = int(SS[s].reserved_s[slot])
        shard_stats.append(d)
    return sol, shard_stats


def host_split_shard(prob, n_shards, shard, owners=None, soc_owners=None, free_owners=None, index_base=0, raw_problem=None,
                     eig_resid=None):
    """proxsdp_host_split_shard: one shard of the library's own split (csrc/shard_split.hpp), everything 0-based.  Returns a
    dict: vars, rows_eq, rows_in, coupling_rows, coupling_owned, A / G (scipy CSC), b, h, c, psd_ids, soc_ids, psd / soc
    (lists of the shard's own variable numbers per cone) and eig_resid (the shard's share of the start vectors `eig_resid`,
    one per PSD cone of the model; empty without them).  raw_problem: a callable that edits the marshalled proxsdp_problem
    before the call (tests of the rejected inputs)."""
    L = lib()
    M = _Marshalled(prob, eig_resid, index_base)
    if raw_problem is not None:
        raw_problem(M.P)
    keep, ptrs = _owner_arrays(owners, soc_owners, free_owners)
    S = ShardIO()
    S.struct_size = C.sizeof(ShardIO)
    call = lambda: _check(L.proxsdp_host_split_shard(C.byref(M.P), int(n_shards), ptrs[0], ptrs[1], ptrs[2], int(shard), C.byref(S)))
    call()                                             # sizes
    sizes = dict(vars=S.n, rows_eq=S.p, rows_in=S.m, coupling_rows=S.n_coupling, coupling_owned=S.n_coupling,
                 A_colptr=S.n + 1, A_rowval=S.nnz_A, A_nzval=S.nnz_A, G_colptr=S.n + 1, G_rowval=S.nnz_G, G_nzval=S.nnz_G,
                 b=S.p, h=S.m, c=S.n, psd_ids=S.n_psd, psd_ptr=S.n_psd + 1, psd_idx=S.len_psd,
                 soc_ids=S.n_soc, soc_ptr=S.n_soc + 1, soc_idx=S.len_soc, eig_resid=S.len_eig)
    out = {}
    for name, t in ShardIO._fields_:
        if name not in sizes:
            continue
        dt = np.float64 if t is pf64 else (np.int32 if name == "coupling_owned" else np.int64)
        out[name] = np.full(max(sizes[name], 1), -7, dtype=dt)
        setattr(S, name, out[name].ctypes.data_as(t))
    call()
    del keep
    out = {k: v[:sizes[k]] for k, v in out.items()}
    n_, p_, m_ = int(S.n), int(S.p), int(S.m)
    res = {k: out[k] for k in ("vars", "rows_eq", "rows_in", "coupling_rows", "coupling_owned", "b", "h", "c", "psd_ids", "soc_ids", "eig_resid")}
    res["A"] = sp.csc_matrix((out["A_nzval"], out["A_rowval"], out["A_colptr"]), shape=(p_, n_))
    res["G"] = sp.csc_matrix((out["G_nzval"], out["G_rowval"], out["G_colptr"]), shape=(m_, n_))
    for kind in ("psd", "soc"):
        ptr, idx = out[kind + "_ptr"], out[kind + "_idx"]
        res[kind] = [idx[ptr[k]:ptr[k + 1]].copy() for k in range(len(ptr) - 1)]
    return res


def host_group_reduce(records, nsum, leave_shard=-1, leave_after=0, timeout_s=0.0):
    """proxsdp_host_group_reduce: records (rounds x shards x width) through the in-process group's barrier + combine, one
    thread per shard.  Returns (out: shards x rounds x width, rounds_done, failed)."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    K, S, w = rec.shape
    out = np.zeros((S, max(K, 1), w))
    done, failed = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    _check(lib().proxsdp_host_group_reduce(S, K, int(nsum), w - int(nsum), _p(rec), int(leave_shard), int(leave_after),
                                           float(timeout_s), _p(out), _p(done, C.POINTER(i32)), _p(failed, C.POINTER(i32))))
    return out[:, :K], done, failed


def coupling_sum(parts, rows, v):
    """proxsdp_hip_coupling_sum: v with v[rows[k]] = ((parts[0][k] + parts[1][k]) + ...) -- the in-process group's kernel"""
    parts = np.ascontiguousarray(parts, dtype=np.float64)
    S, Ln = parts.shape
    rows, vin = _i(rows), _f(v)
    assert len(rows) == Ln
    out = np.zeros_like(vin)
    _check(lib().proxsdp_hip_coupling_sum(_p(parts), S, Ln, _p(rows, pi64), _p(vin), len(vin), _p(out)))
    return out


# ----------------------------------------------------------------- kernel-level entry points
def psd_project(packed, n, target_rank, mode=0, options=None, resid=None):
    L = lib()
    x = _f(packed)
    out = np.zeros_like(x)
    rank, conv, fell = i32(), i32(), i32()
    mineig, nmv = f64(), i64()
    r = _f(resid) if resid is not None else None
    _check(L.proxsdp_hip_psd_project(_p(x), n, target_rank, mode,
                                     C.byref(options) if options is not None else None,
                                     _p(r) if r is not None else None, _p(out),
                                     C.byref(rank), C.byref(mineig), C.byref(nmv), C.byref(conv), C.byref(fell)))
    return out, dict(rank=rank.value, min_eig=mineig.value, nmatvec=nmv.value,
                     converged=conv.value, fell_back=fell.value)


def eigsolve(packed, n, nev, options=None, resid=None, cap=None):
    L = lib()
    x = _f(packed)
    cap = cap or max(2 * nev + 2, 26)
    vals = np.zeros(cap)
    vecs = np.zeros((cap, n))           # row k = k-th vector (column-major n x cap on the C side)
    cnt, conv, nit = i32(), i32(), i32()
    nmv = i64()
    r = _f(resid) if resid is not None else None
    _check(L.proxsdp_hip_eigsolve(_p(x), n, nev, C.byref(options) if options is not None else None,
                                  _p(r) if r is not None else None, cap, _p(vals), _p(vecs),
                                  C.byref(cnt), C.byref(conv), C.byref(nmv), C.byref(nit)))
    k = min(cnt.value, cap)
    return vals[:k].copy(), vecs[:k].T.copy(), dict(count=cnt.value, converged=conv.value,
                                                    nmatvec=nmv.value, numiter=nit.value)


def symv_packed(packed, n, v, repeat=0):
    L = lib()
    x, vv = _f(packed), _f(v)
    y = np.zeros(n)
    ms = f64(0.0)
    _check(L.proxsdp_hip_symv_packed(_p(x), n, _p(vv), _p(y), repeat, C.byref(ms)))
    return (y, ms.value) if repeat else y


def primal_update(x, Mty, c, tau):
    L = lib()
    x, Mty, c = _f(x), _f(Mty), _f(c)
    out = np.zeros_like(x)
    L.proxsdp_hip_primal_update.argtypes = [pf64, pf64, pf64, f64, i64, pf64]
    _check(L.proxsdp_hip_primal_update(_p(x), _p(Mty), _p(c), float(tau), len(x), _p(out)))
    return out


def dual_trial(y, Mx, Mx_old, bh, p, bt, theta):
    L = lib()
    y, Mx, Mx_old, bh = _f(y), _f(Mx), _f(Mx_old), _f(bh)
    out = np.zeros_like(y)
    nrm = f64(0.0)
    L.proxsdp_hip_dual_trial.argtypes = [pf64, pf64, pf64, pf64, i64, i64, f64, f64, pf64, pf64]
    _check(L.proxsdp_hip_dual_trial(_p(y), _p(Mx), _p(Mx_old), _p(bh), int(p), len(y), float(bt), float(theta),
                                    _p(out), C.byref(nrm)))
    return out, nrm.value


def residuals(x, x_old, Mty, Mty_old, c, tau, y, y_old, Mx, Mx_old, bh, p, sigma):
    L = lib()
    a = [_f(v) for v in (x, x_old, Mty, Mty_old, c)]
    b = [_f(v) for v in (y, y_old, Mx, Mx_old, bh)]
    out = np.zeros(9)
    L.proxsdp_hip_residuals.argtypes = [pf64] * 5 + [f64, i64] + [pf64] * 5 + [i64, i64, f64, pf64]
    _check(L.proxsdp_hip_residuals(*[_p(v) for v in a], float(tau), len(a[0]), *[_p(v) for v in b],
                                   int(p), len(b[0]), float(sigma), _p(out)))
    return out


def reconstruct(Z, lam, n, repeat=0, mfma=-1):
    """mfma: -1 the library's choice, 0 scalar-FMA kernel, 1 fp64 MFMA SYRK"""
    L = lib()
    Zc = np.asfortranarray(Z, dtype=np.float64)
    lam = _f(lam)
    r = len(lam)
    out = np.zeros(n * (n + 1) // 2)
    ms = f64(0.0)
    _check(L.proxsdp_hip_reconstruct_kernel(Zc.ctypes.data_as(pf64), _p(lam), n, r, mfma, _p(out), repeat, C.byref(ms)))
    return (out, ms.value) if repeat else out


def factor_residual(packed, n, V, lam, repeat=0):
    """(||X - V diag(lam) V'||_F^2, ||X||_F^2) of X = smat(packed), PLAIN entries (upper triangle column by column, no
    sqrt(2)), by k_factor_residual.  V: (ldv, r) with ldv >= n -- rows n .. ldv-1 are padding the kernel must not read;
    r = 0 is allowed.  repeat > 0: also the mean kernel time in ms."""
    L = lib()
    x = _f(packed)
    lam = _f(lam)
    r = len(lam)
    Vc = np.asfortranarray(np.asarray(V, dtype=np.float64).reshape(-1, r) if r else np.zeros((n, 0)))
    ldv = Vc.shape[0] if r else n
    if len(x) != n * (n + 1) // 2 or (r and ldv < n):
        raise ValueError("factor_residual: packed / V have the wrong shape")
    r2, x2, ms = f64(0.0), f64(0.0), f64(0.0)
    _check(L.proxsdp_hip_factor_residual_kernel(_p(x), n, Vc.ctypes.data_as(pf64) if r else None, ldv,
                                                _p(lam) if r else None, r, C.byref(r2), C.byref(x2), int(repeat), C.byref(ms)))
    return (r2.value, x2.value, ms.value) if repeat else (r2.value, x2.value)


def full_eig_kernel(packed, n, sign=1, repeat=1):
    """full_eig! of one packed block on device-resident data: (X+ packed, ms per call, rank, products per call).
    sign: 0 rocSOLVER dsyevd, 1 sign-function projection (default sign_start_row), 100 + k: sign_start_row = k,
    -1: the solver's automatic engine choice (full_eig_sign = -1)"""
    L = lib()
    xin = _f(packed)
    out = np.zeros(n * (n + 1) // 2)
    ms = f64(0.0)
    rk = i32(0)
    npr = i64(0)
    _check(L.proxsdp_hip_full_eig_kernel(_p(xin), n, int(sign), _p(out), repeat, C.byref(ms), C.byref(rk), C.byref(npr)))
    return out, ms.value, rk.value, npr.value


def spmv(M, x, transpose=False, index_base=0):
    """index_base = 1: colptr and rowval are handed over 1-based, as the Julia shim does"""
    L = lib()
    M = sp.csc_matrix(M, dtype=np.float64)
    M.sort_indices()
    cp, rv, nz = _i(M.indptr) + int(index_base), _i(M.indices) + int(index_base), _f(M.data)
    S = CSC(M.shape[0], M.shape[1], _p(cp, pi64), _p(rv, pi64), _p(nz))
    xin = _f(x)
    out = np.zeros(M.shape[1] if transpose else M.shape[0])
    _check(L.proxsdp_hip_spmv(C.byref(S), int(index_base), 1 if transpose else 0, _p(xin), _p(out)))
    return out


NCAND, NSCAL = 3, 11    # candidates per linesearch batch, scalars per candidate (csrc/pdhg_loop.hip.hpp)


class TrialBatchIO(C.Structure):
    """proxsdp_trial_batch (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64), ("p", i64),
                ("bh", pf64), ("y", pf64), ("Mx", pf64), ("Mx_old", pf64),
                ("x", pf64), ("x_old", pf64), ("Mty_old", pf64), ("roww", pf64),
                ("xold_coef", f64), ("tau_update", f64),
                ("support", i32), ("nc", i32), ("plain", i32), ("c0", i32),
                ("tau", f64 * 3), ("theta", f64 * 3), ("bt", f64 * 3), ("sigma", f64 * 3),
                ("tau_re", f64), ("sigma_re", f64),
                ("y_out", pf64), ("Mty_out", pf64), ("scal", pf64), ("scal_re", pf64),
                ("supp_out", C.POINTER(i32)), ("x_upd", pf64), ("xsave", pf64), ("esv", pf64),
                ("ns", i64), ("gq", i32), ("gx", i32)]


def trial_batch(colptr, rowval, nzval, Q, *, p, bh, y, Mx, Mx_old, x, x_old, Mty_old, c, tau, theta, bt, sigma,
                xold_coef=1.0, support=False, roww=None, plain=False, c0=-1, tau_re=0.0, sigma_re=0.0, tau_update=0.0,
                sharded_rows=False):
    """proxsdp_hip_trial_batch: one batch of len(tau) linesearch candidates through the solver's launches.  M (Q x n) is
    given as raw CSC arrays (0-based) and is used in its storage order.  Returns a dict: y (nc x Q), Mty (nc x ns), scal
    (nc x 11), gq, gx, and -- c0 >= 0 -- scal_re (11); on the support path also supp, x_upd, xsave, esv (2 x ns).
    sharded_rows (general path only): the residual pass of a block-sharded solve's general path, b'y and h'y weighted by
    roww (proxsdp_trial_batch.support = 2); without it they stay unweighted on the general path."""
    if sharded_rows and support:
        raise ValueError("sharded_rows is the general path's switch: the support path always takes the row weights")
    cp, rv, nz = _i(colptr), _i(rowval), _f(nzval)
    n, nc = len(cp) - 1, len(tau)
    rv1, nz1 = (rv, nz) if len(rv) else (np.zeros(1, dtype=np.int64), np.zeros(1))
    S = CSC(int(Q), n, _p(cp, pi64), _p(rv1, pi64), _p(nz1))
    ins = {k: _f(v) for k, v in dict(bh=bh, y=y, Mx=Mx, Mx_old=Mx_old, x=x, x_old=x_old, Mty_old=Mty_old).items()}
    for k, v in ins.items():
        assert len(v) == (n if k in ("x", "x_old", "Mty_old") else Q), k
    cc = _f(c)
    rw = _f(roww) if roww is not None else None
    assert len(cc) == n and (rw is None or len(rw) == Q) and 1 <= nc <= NCAND
    assert len(theta) == len(bt) == len(sigma) == nc
    t = TrialBatchIO()
    t.struct_size = C.sizeof(TrialBatchIO)
    t.p = int(p)
    for k, v in ins.items():
        setattr(t, k, _p(v))
    t.roww = _p(rw) if rw is not None else None
    t.xold_coef, t.tau_update = float(xold_coef), float(tau_update)
    t.support, t.nc, t.plain, t.c0 = (2 if sharded_rows else int(bool(support))), nc, int(bool(plain)), int(c0)
    for k in range(nc):
        t.tau[k], t.theta[k], t.bt[k], t.sigma[k] = float(tau[k]), float(theta[k]), float(bt[k]), float(sigma[k])
    t.tau_re, t.sigma_re = float(tau_re), float(sigma_re)
    out = dict(y=np.zeros((nc, Q)), Mty=np.zeros(nc * n), scal=np.zeros((nc, NSCAL)), scal_re=np.zeros(NSCAL),
               supp=np.zeros(n, dtype=np.int32), x_upd=np.zeros(n), xsave=np.zeros(n), esv=np.zeros(2 * n))
    t.y_out, t.Mty_out, t.scal, t.scal_re = _p(out["y"]), _p(out["Mty"]), _p(out["scal"]), _p(out["scal_re"])
    t.supp_out, t.x_upd, t.xsave, t.esv = _p(out["supp"], C.POINTER(i32)), _p(out["x_upd"]), _p(out["xsave"]), _p(out["esv"])
    L = lib()
    L.proxsdp_hip_trial_batch.argtypes = [C.POINTER(CSC), i32, pf64, C.POINTER(TrialBatchIO)]
    _check(L.proxsdp_hip_trial_batch(C.byref(S), 0, _p(cc), C.byref(t)))
    ns = int(t.ns)
    res = dict(y=out["y"], Mty=out["Mty"][:nc * ns].reshape(nc, ns), scal=out["scal"], gq=int(t.gq), gx=int(t.gx))
    if c0 >= 0:
        res["scal_re"] = out["scal_re"]
    if support:
        res.update(supp=out["supp"][:ns].copy(), x_upd=out["x_upd"], xsave=out["xsave"][:ns].copy(),
                   esv=out["esv"][:2 * ns].reshape(2, ns).copy())
    return res


def cone_tail(x, soc_off, soc_len, one_off):
    """proxsdp_hip_cone_tail: (x after the SOC projection, SOC gap before, SOC gap after, x after the 1x1 clamp, min_eig)"""
    x = _f(x)
    so, sl, oo = _i(soc_off), np.ascontiguousarray(soc_len, dtype=np.int32), _i(one_off)
    ns_, no_ = len(so), len(oo)
    assert len(sl) == ns_
    pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)
    so, sl, oo = pad(so), pad(sl), pad(oo)
    x_soc, x_cl = np.zeros_like(x), np.zeros_like(x)
    g0, g1, me = np.zeros(max(ns_, 1)), np.zeros(max(ns_, 1)), np.zeros(max(no_, 1))
    L = lib()
    L.proxsdp_hip_cone_tail.argtypes = [pf64, i64, pi64, C.POINTER(i32), i32, pi64, i32, pf64, pf64, pf64, pf64, pf64]
    _check(L.proxsdp_hip_cone_tail(_p(x), len(x), _p(so, pi64), _p(sl, C.POINTER(i32)), ns_, _p(oo, pi64), no_,
                                   _p(x_soc), _p(g0), _p(g1), _p(x_cl), _p(me)))
    return x_soc, g0[:ns_], g1[:ns_], x_cl, me[:no_]


BLOCK_CLASSES = ("1x1", "small-jacobi", "small-sign", "large")       # proxsdp_project_cones.block_class


class ProjectConesIO(C.Structure):
    """proxsdp_project_cones (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64),
                ("x", pf64), ("x_out", pf64),
                ("block_off", pi64), ("block_side", C.POINTER(i32)), ("block_class", C.POINTER(i32)),
                ("rank", pi64), ("min_eig", pf64), ("sweeps", C.POINTER(i32)),
                ("batched_small_eigs", i64), ("full_eigs", i64), ("full_eigs_sign", i64),
                ("sign_short_pass", i64), ("sign_short_fail", i64)]


def project_cones(prob, x, options=None):
    """proxsdp_hip_project_cones: ONE psd_projection of the n-vector x (solver order and scaling) through the solver's own set-up
    and launch code; the problem gives the cone layout only.  Returns a dict: x (projected), and per PSD block offset, side,
    cls (a name of BLOCK_CLASSES), rank, min_eig, sweeps (-1 where no Jacobi ran); stats (the five counters of the call)."""
    M = _Marshalled(prob)
    x = _f(x)
    assert len(x) == M.P.n
    nb = max(len(prob.psd), 1)
    pi32 = C.POINTER(i32)
    out = np.zeros_like(x)
    off, rank = np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
    side, cls, sweeps = (np.zeros(nb, dtype=np.int32) for _ in range(3))
    me = np.zeros(nb)
    t = ProjectConesIO()
    t.struct_size = C.sizeof(ProjectConesIO)
    t.x, t.x_out = _p(x), _p(out)
    t.block_off, t.block_side, t.block_class = _p(off, pi64), _p(side, pi32), _p(cls, pi32)
    t.rank, t.min_eig, t.sweeps = _p(rank, pi64), _p(me), _p(sweeps, pi32)
    _check(lib().proxsdp_hip_project_cones(C.byref(M.P), C.byref(options) if options is not None else None, C.byref(t)))
    k = len(prob.psd)
    return dict(x=out, offset=off[:k], side=side[:k], cls=[BLOCK_CLASSES[c] for c in cls[:k]], rank=rank[:k], min_eig=me[:k],
                sweeps=sweeps[:k],
                stats={f: getattr(t, f) for f in ("batched_small_eigs", "full_eigs", "full_eigs_sign", "sign_short_pass", "sign_short_fail")})


SYM_EPILOGUES = {"plain": 0, "poly": 1, "final": 2, "final_res": 3}    # proxsdp_sym_product.epilogue
SYM_SENTINEL = -7.25e300                                                 # default prefill of the outputs: no product comes near it


class SymProductIO(C.Structure):
    """proxsdp_sym_product (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64),
                ("n", i32), ("tile", i32), ("epilogue", i32), ("use_dsc", i32),
                ("P", pf64), ("Q", pf64), ("Y", pf64),
                ("ca", f64), ("cb", f64), ("cc", f64), ("dsc", f64 * 3),
                ("xold", pf64), ("mask", C.POINTER(C.c_uint32)), ("mask_words", i64), ("mask_off", i64),
                ("sentinel", f64),
                ("T", pf64), ("part", pf64), ("xp", pf64), ("respart", pf64),
                ("ld", i32), ("grid", i32)]


def sym_product(P, Q, *, tile, epilogue="plain", Y=None, ca=0.0, cb=0.0, cc=0.0, dsc=None, xold=None, mask=None,
                mask_off=0, sentinel=SYM_SENTINEL, want_part=True):
    """proxsdp_hip_sym_product: ONE product of the sign iteration through Solver::sym_gemm, on tiles of side `tile` (32, 48, 64).
    P, Q (and Y for "poly"): symmetric n x n.  Returns a dict: ld, grid, and -- "plain" / "poly" -- T (ld x ld, padding
    included; entries the launch did not write hold `sentinel`) and part (grid slots, None without want_part); -- "final" /
    "final_res" -- xp (packed), part (trace partials) and, for "final_res", respart (2 x grid)."""
    Pm = np.asfortranarray(P, dtype=np.float64)
    Qm = np.asfortranarray(Q, dtype=np.float64)
    n = Pm.shape[0]
    assert Pm.shape == (n, n) == Qm.shape
    epi = SYM_EPILOGUES[epilogue]
    ld = 64 * ((n + 63) // 64)
    cap = (ld // 32 + 1) ** 2 // 2 + 8
    t = SymProductIO()
    t.struct_size = C.sizeof(SymProductIO)
    t.n, t.tile, t.epilogue, t.use_dsc = n, int(tile), epi, int(dsc is not None)
    t.P, t.Q = _p(Pm), _p(Qm)
    if epi == 1:
        Ym = np.asfortranarray(Y, dtype=np.float64)
        assert Ym.shape == (n, n)
        t.Y = _p(Ym)
    t.ca, t.cb, t.cc = float(ca), float(cb), float(cc)
    for k in range(3):
        t.dsc[k] = float(dsc[k]) if dsc is not None else 0.0
    t.sentinel = float(sentinel)
    N = n * (n + 1) // 2
    out = {}
    if epi < 2:
        out["T"] = np.zeros((ld, ld), order="F")
        t.T = _p(out["T"])
    else:
        out["xp"] = np.zeros(N)
        t.xp = _p(out["xp"])
    if want_part or epi >= 2:
        part = np.zeros(cap)
        t.part = _p(part)
    if epi == 3:
        xo = _f(xold)
        mk = np.ascontiguousarray(mask, dtype=np.uint32)
        assert len(xo) == N
        t.xold, t.mask, t.mask_words, t.mask_off = _p(xo), _p(mk, C.POINTER(C.c_uint32)), len(mk), int(mask_off)
        resp = np.zeros(2 * cap)
        t.respart = _p(resp)
    _check(lib().proxsdp_hip_sym_product(C.byref(t)))
    assert t.ld == ld and t.grid <= cap
    out.update(ld=ld, grid=int(t.grid), part=part[:t.grid].copy() if (want_part or epi >= 2) else None)
    if epi == 3:
        out["respart"] = resp[:2 * t.grid].reshape(2, t.grid).copy()
    return out


def sign_unpack(packed, n, sentinel=SYM_SENTINEL):
    """proxsdp_hip_sign_unpack: (A, sc) -- A (ld x ld) as k_unpack_sym leaves a matrix prefilled with `sentinel`, sc[16] the
    device scalars after the first product (sc[0] = 1/f^2, sc[6] = f, sc[1] = 1/s, sc[4] = s, sc[8..10] = {1, 1/g, 1/g^2})."""
    xin = _f(packed)
    assert len(xin) == n * (n + 1) // 2
    ld = 64 * ((n + 63) // 64)
    A = np.zeros((ld, ld), order="F")
    sc = np.zeros(16)
    _check(lib().proxsdp_hip_sign_unpack(_p(xin), n, float(sentinel), _p(A), _p(sc)))
    return A, sc


pu32 = C.POINTER(C.c_uint32)
ROTATE_FORMS = {0: "none", 1: "scalar", 2: "mfma", 3: "wide"}            # PROXSDP_ROTATE_*
RESPART_GUARD = 16                                                        # slots asked for behind 2 grid: nothing may write them


class ReconstructFusedIO(C.Structure):
    """proxsdp_reconstruct_fused (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64),
                ("n", i32), ("r", i32), ("ldz", i32), ("mfma", i32),
                ("Z", pf64), ("lam", pf64), ("xold", pf64),
                ("mask", pu32), ("mask_words", i64), ("mask_off", i64),
                ("respart_cap", i64), ("sentinel", f64),
                ("xp", pf64), ("respart", pf64),
                ("grid", i32), ("kernel", i32)]


class RotationIO(C.Structure):
    """proxsdp_rotation (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64),
                ("n", i32), ("K", i32), ("ncols", i32), ("Kv", i32), ("copy_src", i32), ("copy_dst", i32), ("wide", i32),
                ("out_cols", i32),
                ("V", pf64), ("U", pf64), ("sentinel", f64),
                ("out", pf64),
                ("npad", i32), ("form", i32), ("launches", i32), ("reserved", i32)]


class TailCopyIO(C.Structure):
    """proxsdp_tail_copy (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64),
                ("N", i64), ("start", i64),
                ("xin", pf64), ("mask", pu32), ("mask_words", i64),
                ("wgs", i32), ("reserved", i32), ("sentinel", f64),
                ("xout", pf64), ("respart", pf64)]


def reconstruct_fused(Z, lam, n, *, mfma=-1, xold=None, mask=None, mask_off=0, sentinel=SYM_SENTINEL):
    """proxsdp_hip_reconstruct_fused: ONE reconstruction through Solver::launch_reconstruct.  Z: (ldz, r) with ldz >= n (rows
    n .. ldz-1 are padding the kernels must not read), lam: (r,).  xold (packed) with mask / mask_off: the fused launch of the
    support path; without xold the unfused one.  Returns a dict: xp (packed), respart (2 x grid), guard (the RESPART_GUARD slots
    behind them), grid, kernel ("packed" / "mfma"); what the launch did not write holds `sentinel`."""
    Zm = np.asfortranarray(Z, dtype=np.float64)
    ldz, r = Zm.shape
    lm = _f(lam)
    assert len(lm) == r
    N = n * (n + 1) // 2
    nt = (n + 63) // 64
    grid = 8 * ((nt * (nt + 1) // 2 + 7) // 8) if n >= 1 else 8
    t = ReconstructFusedIO()
    t.struct_size = C.sizeof(ReconstructFusedIO)
    t.n, t.r, t.ldz, t.mfma = n, r, ldz, int(mfma)
    if r > 0:
        t.Z, t.lam = _p(Zm), _p(lm)
    if xold is not None:
        xo = _f(xold)
        mk = np.ascontiguousarray(mask, dtype=np.uint32)
        assert len(xo) == N
        t.xold, t.mask, t.mask_words, t.mask_off = _p(xo), _p(mk, pu32), len(mk), int(mask_off)
    xp = np.zeros(max(N, 1))
    resp = np.zeros(2 * grid + RESPART_GUARD)
    t.respart_cap, t.sentinel = len(resp), float(sentinel)
    t.xp, t.respart = _p(xp), _p(resp)
    _check(lib().proxsdp_hip_reconstruct_fused(C.byref(t)))
    assert t.grid == grid
    return dict(xp=xp[:N], respart=resp[:2 * grid].reshape(2, grid).copy(), guard=resp[2 * grid:].copy(), grid=grid,
                kernel=("packed", "mfma")[t.kernel])


def rotate(V, U, K, *, copy_src=-1, copy_dst=0, wide=0, out_cols=None, sentinel=SYM_SENTINEL):
    """proxsdp_hip_rotate: out[:, :ncols] = V[:, :K] U through Solver::rotate.  V: (n, Kv), U: (K, ncols).  Returns a dict:
    out (npad, out_cols), form ("scalar" / "mfma" / "wide" / "none"), launches."""
    Vm = np.asfortranarray(V, dtype=np.float64)
    Um = np.asfortranarray(U, dtype=np.float64)
    n, Kv = Vm.shape
    ncols = Um.shape[1]
    assert Um.shape[0] == K
    if out_cols is None:
        out_cols = max(ncols, copy_dst + 1 if copy_src >= 0 else 0, 1)
    npad = 64 * ((n + 63) // 64)
    out = np.zeros((npad, max(out_cols, 1)), order="F")
    t = RotationIO()
    t.struct_size = C.sizeof(RotationIO)
    t.n, t.K, t.ncols, t.Kv, t.copy_src, t.copy_dst, t.wide, t.out_cols = n, int(K), ncols, Kv, int(copy_src), int(copy_dst), int(wide), int(out_cols)
    t.V, t.sentinel, t.out = _p(Vm), float(sentinel), _p(out)
    if Um.size:
        t.U = _p(Um)
    _check(lib().proxsdp_hip_rotate(C.byref(t)))
    assert t.npad == npad
    return dict(out=out, form=ROTATE_FORMS[t.form], launches=int(t.launches))


def tail_copy(xin, start, mask, wgs, sentinel=SYM_SENTINEL):
    """proxsdp_hip_tail_copy: k_tail_copy_res through Solver::launch_tail_copy on `wgs` workgroups.  Returns (xout, respart):
    xout (N, prefilled with `sentinel`), respart (2, wgs)."""
    xi = _f(xin)
    mk = np.ascontiguousarray(mask, dtype=np.uint32)
    t = TailCopyIO()
    t.struct_size = C.sizeof(TailCopyIO)
    t.N, t.start, t.wgs, t.sentinel = len(xi), int(start), int(wgs), float(sentinel)
    xout = np.zeros(len(xi))
    resp = np.zeros(2 * max(int(wgs), 1))
    t.xin, t.mask, t.mask_words, t.xout, t.respart = _p(xi), _p(mk, pu32), len(mk), _p(xout), _p(resp)
    _check(lib().proxsdp_hip_tail_copy(C.byref(t)))
    return xout, resp.reshape(2, -1).copy()


LZ_ENGINES = {0: "step", 1: "block1", 2: "wide"}                          # PROXSDP_LZ_ENGINE_*
LZ_INFO = 12                                                              # PROXSDP_LZ_INFO
pi32 = C.POINTER(i32)


class LanczosCyclesIO(C.Structure):
    """proxsdp_lanczos_cycles (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64),
                ("n", i32), ("nev", i32), ("max_cycles", i32), ("cols", i32), ("ldv", i32), ("reserved", i32),
                ("packed", pf64), ("opt", C.POINTER(Options)), ("resid", pf64), ("sentinel", f64),
                ("info", pi32), ("V", pf64), ("alphas", pf64), ("betas", pf64), ("D", pf64), ("f", pf64),
                ("npad", i32), ("krylovdim", i32), ("cycles", i32), ("reserved2", i32)]


def _krylov_dim(o, nev):
    return max(2 * int(nev) + 1, int(get_option(o, "eigsolver_min_lanczos")))


def _lanczos_cycles_io(packed, n, nev, max_cycles, o, resid, sentinel, kd):
    """proxsdp_lanczos_cycles for a run of Krylov dimension kd, filled in, and the function that decodes it after the call
    (it keeps the arrays alive)"""
    x = _f(packed)
    assert len(x) == n * (n + 1) // 2
    cols, npad, mc = kd + 1, 64 * ((n + 63) // 64), max(int(max_cycles), 1)
    t = LanczosCyclesIO()
    t.struct_size = C.sizeof(LanczosCyclesIO)
    t.n, t.nev, t.max_cycles, t.cols, t.ldv = int(n), int(nev), int(max_cycles), cols, npad
    t.packed, t.opt, t.sentinel = _p(x), C.pointer(o), float(sentinel)
    r = _f(resid) if resid is not None else None
    if r is not None:
        assert len(r) == n
        t.resid = _p(r)
    info = np.zeros((mc, LZ_INFO), dtype=np.int32)
    V = np.zeros((mc, cols, npad))
    al, be, D, f = (np.zeros((mc, cols)) for _ in range(4))
    t.info, t.V, t.alphas, t.betas, t.D, t.f = _p(info, pi32), _p(V), _p(al), _p(be), _p(D), _p(f)
    keep = (x, o, r)

    def decode():
        assert t.npad == npad and t.krylovdim == kd and keep is not None
        cyc = [dict(kfirst=int(info[c, 0]), K=int(info[c, 1]), stop=int(info[c, 2]), engine=LZ_ENGINES[int(info[c, 3])],
                    split=bool(info[c, 4]), speculated=bool(info[c, 5]), merge_on_device=bool(info[c, 6]),
                    split_ready=bool(info[c, 7]), kept_compared=bool(info[c, 8]), kept_differ=int(info[c, 9]), V=V[c].T, alphas=al[c], betas=be[c], D=D[c], f=f[c])
               for c in range(t.cycles)]
        return dict(npad=npad, krylovdim=kd, cycles=cyc, untouched=dict(info=info[t.cycles:], V=V[t.cycles:], alphas=al[t.cycles:]))
    return t, decode


def lanczos_cycles(packed, n, nev, max_cycles, options=None, resid=None, sentinel=SYM_SENTINEL):
    """proxsdp_hip_lanczos_cycles: every cycle of one run of Solver::lanczos, ended by the driver after max_cycles.  Returns a
    dict: npad, krylovdim, and `cycles`, one dict per cycle the driver ran: kfirst, K (Kend), stop, engine ("step" / "block1" /
    "wide"), split, speculated, merge_on_device, split_ready, kept_compared / kept_differ (the kept columns against a repeat of
    the restart rotation: entries whose bits differ), V (npad, krylovdim + 1: the whole basis buffer), alphas, betas,
    D, f (krylovdim + 1 each; what the cycle did not write holds `sentinel`)."""
    o = options if options is not None else default_options()
    t, decode = _lanczos_cycles_io(packed, n, nev, max_cycles, o, resid, sentinel, _krylov_dim(o, nev))
    _check(lib().proxsdp_hip_lanczos_cycles(C.byref(t)))
    return decode()


OP_INFO = 16                                                              # PROXSDP_OP_INFO
OP_RLD = 128                                                              # the stride of the records of F'v (probe_tpart)


class OperatorCyclesIO(C.Structure):
    """proxsdp_operator_cycles (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64),
                ("n", i32), ("nev", i32), ("max_cycles", i32), ("cols", i32), ("ldv", i32), ("rp", i32),
                ("f_first", i32), ("no_factors", i32), ("ns", i64),
                ("support", pi32), ("esv", pf64), ("F", pf64), ("lam", pf64), ("opt", C.POINTER(Options)), ("resid", pf64),
                ("probe_v", pf64), ("sentinel", f64),
                ("info", pi32), ("V", pf64), ("alphas", pf64), ("betas", pf64), ("D", pf64), ("f", pf64),
                ("probe_ev", pf64), ("probe_tpart", pf64), ("probe_apart", pf64),
                ("npad", i32), ("krylovdim", i32), ("cycles", i32), ("ell_w", i32), ("overflow_rows", i32), ("reserved", i32)]


def _operator_cycles_io(n, support, values, F, lam, nev, max_cycles, o, resid, no_factors, f_first, other_half, probe_v, sentinel, kd):
    """proxsdp_operator_cycles for a run of Krylov dimension kd, filled in, and the function that decodes it after the call
    (it keeps the arrays alive)"""
    supp = np.ascontiguousarray(support, dtype=np.int32)
    vals = _f(values)
    ns = len(supp)
    assert len(vals) == ns
    oth = np.full(ns, np.nan) if other_half is None else _f(other_half)
    assert len(oth) == ns
    esv = np.ascontiguousarray(np.concatenate([oth, vals] if no_factors else [vals, oth]))
    Fm = np.asfortranarray(np.asarray(F, dtype=np.float64).reshape(n, -1))
    lm = _f(lam)
    rp = Fm.shape[1]
    assert len(lm) == rp
    cols, npad, mc = kd + 1, 64 * ((n + 63) // 64), max(int(max_cycles), 1)
    nt = npad // 64
    t = OperatorCyclesIO()
    t.struct_size = C.sizeof(OperatorCyclesIO)
    t.n, t.nev, t.max_cycles, t.cols, t.ldv, t.rp = int(n), int(nev), int(max_cycles), cols, npad, rp
    t.f_first, t.no_factors, t.ns = int(f_first), int(bool(no_factors)), ns
    Ff = Fm.ravel(order="F")
    if ns > 0:
        t.support, t.esv = _p(supp, pi32), _p(esv)
    if rp > 0:
        t.F, t.lam = _p(Ff), _p(lm)
    t.opt, t.sentinel = C.pointer(o), float(sentinel)
    r = _f(resid) if resid is not None else None
    if r is not None:
        assert len(r) == n
        t.resid = _p(r)
    pv = _f(probe_v) if probe_v is not None else None
    pev, ptp, pap = np.zeros(npad), np.zeros((nt, OP_RLD)), np.zeros(nt)
    if pv is not None:
        assert len(pv) == n
        t.probe_v, t.probe_ev, t.probe_tpart, t.probe_apart = _p(pv), _p(pev), _p(ptp), _p(pap)
    info = np.zeros((mc, OP_INFO), dtype=np.int32)
    V = np.zeros((mc, cols, npad))
    al, be, D, f = (np.zeros((mc, cols)) for _ in range(4))
    t.info, t.V, t.alphas, t.betas, t.D, t.f = _p(info, pi32), _p(V), _p(al), _p(be), _p(D), _p(f)
    keep = (supp, esv, Ff, lm, o, r, pv)

    def decode():
        assert keep is not None
        assert t.npad == npad and t.krylovdim == kd
        cyc = [dict(kfirst=int(info[c, 0]), K=int(info[c, 1]), stop=int(info[c, 2]), engine=LZ_ENGINES[int(info[c, 3])],
                    split=bool(info[c, 4]), speculated=bool(info[c, 5]), merge_on_device=bool(info[c, 6]),
                    split_ready=bool(info[c, 7]), kept_compared=bool(info[c, 8]), kept_differ=int(info[c, 9]),
                    fop=int(info[c, 10]), owner=bool(info[c, 11]), nchp=int(info[c, 12]), ell_w=int(info[c, 13]),
                    overflow_rows=int(info[c, 14]), ell_in_lds=None if info[c, 15] < 0 else bool(info[c, 15]),
                    V=V[c].T, alphas=al[c], betas=be[c], D=D[c], f=f[c])
               for c in range(t.cycles)]
        out = dict(npad=npad, krylovdim=kd, cycles=cyc, ell_w=int(t.ell_w), overflow_rows=int(t.overflow_rows),
                   untouched=dict(info=info[t.cycles:], V=V[t.cycles:], alphas=al[t.cycles:]))
        if pv is not None:
            out["probe"] = dict(ev=pev, tpart=ptp, apart=pap)
        return out
    return t, decode


def operator_cycles(n, support, values, F, lam, nev, max_cycles, options=None, resid=None, no_factors=False, f_first=0,
                    other_half=None, probe_v=None, sentinel=SYM_SENTINEL):
    """proxsdp_hip_operator_cycles: every cycle of one run of Solver::lanczos on the operator form A v = F (lam o F'v) + E v.
    support: ascending packed indices of E's entries; values: theirs in svec units (off-diagonals carry the sqrt(2)); they go
    into the half of the support-value array that the form reads (no_factors: the second), `other_half` (default NaN) into
    the other.  F (n, rp), lam (rp).  Returns lanczos_cycles' dict; every cycle has besides: fop (the mat-vecs it ran on the
    operator-form kernels), owner, nchp, ell_w, overflow_rows, ell_in_lds (None on the step kernels); the dict has ell_w,
    overflow_rows and, with probe_v, probe = dict(ev (npad), tpart (nt, 128), apart (nt)) of one mat-vec launch."""
    o = options if options is not None else default_options()
    t, decode = _operator_cycles_io(n, support, values, F, lam, nev, max_cycles, o, resid, no_factors, f_first, other_half, probe_v,
                                    sentinel, _krylov_dim(o, nev))
    _check(lib().proxsdp_hip_operator_cycles(C.byref(t)))
    return decode()


class PositivePartIO(C.Structure):
    """proxsdp_positive_part (include/proxsdp_hip.h)"""
    _fields_ = [("struct_size", i64),
                ("packed_run", C.POINTER(LanczosCyclesIO)), ("operator_run", C.POINTER(OperatorCyclesIO)),
                ("ws_rank", i32), ("cap", i32), ("run", i32), ("cert_steps", i32), ("npos_in", i32), ("reserved", i32),
                ("locked", pf64), ("locked_vals", pf64),
                ("converged", i32), ("count", i32), ("numiter", i32), ("warm", i32), ("vals", pf64), ("Z", pf64),
                ("cert_ran", i32), ("npos", i32), ("steps", i32), ("stop", i32), ("kstop", i32), ("reserved2", i32),
                ("differ", i64), ("matvecs", i64), ("theta_max", f64), ("scale", f64), ("posres", f64),
                ("cert_alphas", pf64), ("cert_betas", pf64), ("basis", pf64), ("resid2", pf64)]


def positive_part_dims(n, nev, ws_rank, options=None):
    """(cap, krylovdim) of a positive-part run for nev pairs in a workspace sized for ws_rank pairs, as the header states them"""
    o = options if options is not None else default_options()
    kmin = int(get_option(o, "eigsolver_min_lanczos"))
    k10 = int(get_option(o, "full_eig_lanczos_kdim10"))
    cap = min(max(2 * min(max(int(ws_rank), 2), int(n)) + 1, kmin), 255) + 1
    return cap, min(min(cap, 256) - 1, max(max(2 * int(nev) + 1, kmin), int(nev) * (k10 if k10 > 0 else 30) // 10 + 8))


def positive_part(n, nev, ws_rank, max_cycles=1, packed=None, operator=None, options=None, resid=None, run=True, cert_steps=0,
                  locked=None, locked_vals=None, sentinel=SYM_SENTINEL):
    """proxsdp_hip_positive_part: one positive-part run of Solver::lanczos through the per-cycle observer, then
    Solver::lanczos_certificate.  The block: `packed` (lanczos_cycles' argument) or `operator`, a dict of operator_cycles'
    arguments (support, values, F, lam; no_factors, f_first, other_half).  locked (n, npos) / locked_vals: the pairs the
    certificate locks in place of the run's.  Returns the wrapped entry's dict and: cap; with run: converged, count, numiter,
    warm, vals (count), Z (npad, count); with cert_steps >= 2, cert = dict(ran, npos, steps, stop, kstop, theta_max, scale,
    posres, differ, matvecs, alphas, betas (cap each), basis (npad, cap), resid2 (npad))."""
    o = options if options is not None else default_options()
    cap, kd = positive_part_dims(n, nev, ws_rank, o)
    npad = 64 * ((n + 63) // 64)
    p = PositivePartIO()
    p.struct_size = C.sizeof(PositivePartIO)
    p.ws_rank, p.cap, p.run, p.cert_steps, p.npos_in = int(ws_rank), cap, int(bool(run)), int(cert_steps), -1
    if locked is not None:
        Lk = np.asfortranarray(np.asarray(locked, dtype=np.float64).reshape(n, -1))
        lv = _f(locked_vals)
        assert len(lv) == Lk.shape[1]
        Lf = Lk.ravel(order="F")
        p.npos_in = Lk.shape[1]
        if p.npos_in > 0:
            p.locked, p.locked_vals = _p(Lf), _p(lv)
    vals, al, be = np.zeros(cap), np.zeros(cap), np.zeros(cap)
    Z, basis, r2 = np.zeros((cap, npad)), np.zeros((cap, npad)), np.zeros(npad)
    p.vals, p.Z, p.cert_alphas, p.cert_betas, p.basis, p.resid2 = _p(vals), _p(Z), _p(al), _p(be), _p(basis), _p(r2)

    if packed is not None:
        t, decode = _lanczos_cycles_io(packed, n, nev, max_cycles, o, resid, sentinel, kd)
        p.packed_run = C.pointer(t)
    else:
        op = dict(operator)
        t, decode = _operator_cycles_io(n, op["support"], op["values"], op["F"], op["lam"], nev, max_cycles, o, resid,
                                        op.get("no_factors", False), op.get("f_first", 0), op.get("other_half"), op.get("probe_v"),
                                        sentinel, kd)
        p.operator_run = C.pointer(t)
    _check(lib().proxsdp_hip_positive_part(C.byref(p)))
    out = decode()
    out.update(cap=cap, converged=bool(p.converged), count=int(p.count), numiter=int(p.numiter), warm=bool(p.warm),
               vals=vals[:p.count].copy(), Z=Z[:p.count].T.copy())
    if cert_steps >= 2:
        out["cert"] = dict(ran=bool(p.cert_ran), npos=int(p.npos), steps=int(p.steps), stop=int(p.stop), kstop=int(p.kstop),
                           theta_max=float(p.theta_max), scale=float(p.scale), posres=float(p.posres), differ=int(p.differ),
                           matvecs=int(p.matvecs), alphas=al, betas=be, basis=basis.T, resid2=r2)
    return out


def block1_lds_doubles(nt, fop, xN=0, ell_w_lds=0):
    """proxsdp_host_block1_lds_doubles: the doubles of dynamic LDS k_lz_block1 asks for (b1_lds_plan); host only"""
    r = int(lib().proxsdp_host_block1_lds_doubles(int(nt), int(bool(fop)), int(xN), int(ell_w_lds)))
    if r < 0:
        raise ValueError("block1_lds_doubles: nt must be 1 .. 8, sizes non-negative, ell_w_lds <= 32")
    return r


def dense_scaling(prob, options=None):
    """proxsdp_hip_dense_scaling: the Init section of a solve with a dense A.  Returns (E, D, frob, sigma_max,
    equilibrated); sigma_max is 0 unless options.approx_norm = 0."""
    M = _Marshalled(prob)
    Q = M.P.p + M.P.m
    E, D = np.zeros(max(Q, 1)), np.zeros(max(M.P.n, 1))
    fro, sig, eq = f64(), f64(), i32()
    _check(lib().proxsdp_hip_dense_scaling(C.byref(M.P), C.byref(options) if options is not None else None,
                                           _p(E), _p(D), C.byref(fro), C.byref(sig), C.byref(eq)))
    return E[:Q], D[:M.P.n], fro.value, sig.value, bool(eq.value)


# ----------------------------------------------------------------- host-only helpers (no GPU)
def host_symeig(A, threads=-1):
    """threads: -1 the library's choice (helper threads from k >= 96), 0 serial -- bit-identical results"""
    L = lib()
    a = np.asfortranarray(A, dtype=np.float64).copy(order="F")
    k = a.shape[0]
    d = np.zeros(k)
    _check(L.proxsdp_host_symeig_threads(k, a.ctypes.data_as(pf64), _p(d), threads))
    return d, a


def host_symeig_arrow(D, f, al, be):
    """Two-phase eigen-decomposition of a thick-restarted Rayleigh quotient (see the header)."""
    L = lib()
    D, f, al, be = _f(D), _f(f), _f(al), _f(be)
    K, m = len(al), len(D)
    U = np.zeros((K, K), order="F")
    d = np.zeros(K)
    L.proxsdp_host_symeig_arrow.argtypes = [i32, i32, pf64, pf64, pf64, pf64, pf64, pf64]
    _check(L.proxsdp_host_symeig_arrow(K, m, _p(D), _p(f), _p(al), _p(be), U.ctypes.data_as(pf64), _p(d)))
    return d, U


def host_start_vector(n, seed=1234, init=3):
    out = np.zeros(n)
    _check(lib().proxsdp_host_start_vector(n, seed, init, _p(out)))
    return out


def host_symeig_split(D, f, al, be, k1, threads=0):
    """proxsdp_host_symeig_split: eigen-decomposition of the restarted Rayleigh quotient (as host_symeig_arrow) by a
    split at k1 + rank-one merge.  Returns (d ascending, U, info dict)."""
    D = _f(D); f = _f(f); al = _f(al); be = _f(be)
    K, m = len(al), len(D)
    U = np.zeros((K, K))
    d = np.zeros(K)
    info = (i32 * 3)()
    L = lib()
    L.proxsdp_host_symeig_split_threads.argtypes = [i32, i32, i32, pf64, pf64, pf64, pf64, i32, pf64, pf64, C.POINTER(i32)]
    _check(L.proxsdp_host_symeig_split_threads(K, m, int(k1), _p(D) if m else None, _p(f) if m else None, _p(al), _p(be),
                                               int(threads), _p(U), _p(d), info))
    return d, U.T.copy(), dict(nondeflated=info[0], deflated=info[1], max_secular_iterations=info[2])


def device_symeig_split(D, f, al, be, k1):
    """proxsdp_device_symeig_split: host_symeig_split with the rank-one merge run by the device kernels the Lanczos driver
    uses (options.device_eig_merge).  Returns (d ascending, U, info dict); needs a HIP device."""
    D = _f(D); f = _f(f); al = _f(al); be = _f(be)
    K, m = len(al), len(D)
    U = np.zeros((K, K))
    d = np.zeros(K)
    info = (i32 * 3)()
    L = lib()
    L.proxsdp_device_symeig_split.argtypes = [i32, i32, i32, pf64, pf64, pf64, pf64, pf64, pf64, C.POINTER(i32)]
    L.proxsdp_device_symeig_split.restype = C.c_int
    _check(L.proxsdp_device_symeig_split(K, m, int(k1), _p(D) if m else None, _p(f) if m else None, _p(al), _p(be),
                                         _p(U), _p(d), info))
    return d, U.T.copy(), dict(nondeflated=info[0], deflated=info[1], max_secular_iterations=info[2])


def host_merge_plan(D, f, al, be, k1, with_qf):
    """proxsdp_host_merge_plan: the split at k1 and Rank1Merge::plan() with or without Qf.  Returns a dict: Q1, Q2 (the two
    parts' eigenvectors), Qf (None without it), d, z, colsrc, nd, rots = [(pj, j, c, s), ...], deflated."""
    D = _f(D); f = _f(f); al = _f(al); be = _f(be)
    K, m = len(al), len(D)
    k1 = int(k1); k2 = K - k1
    Q1 = np.zeros((k1, k1)); Q2 = np.zeros((k2, k2)); Qf = np.zeros((K, K))
    d = np.zeros(K); z = np.zeros(K)
    colsrc = np.zeros(K, dtype=np.int32); nd = np.zeros(K, dtype=np.int32)
    ridx = np.zeros(2 * K, dtype=np.int32); rcs = np.zeros(2 * K)
    counts = (i32 * 3)()
    pi32 = C.POINTER(i32)
    L = lib()
    L.proxsdp_host_merge_plan.argtypes = [i32, i32, i32, pf64, pf64, pf64, pf64, i32, pf64, pf64, pf64, pf64, pf64,
                                          pi32, pi32, pi32, pf64, pi32]
    L.proxsdp_host_merge_plan.restype = C.c_int
    _check(L.proxsdp_host_merge_plan(K, m, k1, _p(D) if m else None, _p(f) if m else None, _p(al), _p(be), int(bool(with_qf)),
                                     _p(Q1), _p(Q2), _p(Qf), _p(d), _p(z), colsrc.ctypes.data_as(pi32), nd.ctypes.data_as(pi32),
                                     ridx.ctypes.data_as(pi32), _p(rcs), counts))
    k, ndf, nrot = counts[0], counts[1], counts[2]
    rots = [(int(ridx[2 * q]), int(ridx[2 * q + 1]), float(rcs[2 * q]), float(rcs[2 * q + 1])) for q in range(nrot)]
    return dict(Q1=Q1.T.copy(), Q2=Q2.T.copy(), Qf=Qf.T.copy() if with_qf else None, d=d, z=z, colsrc=colsrc.copy(),
                nd=nd[:k].copy(), rots=rots, deflated=ndf)


def host_preprocess(prob, index_base=0):
    M = _Marshalled(prob, index_base=index_base)
    n = prob.n
    order, inv = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    cs = np.zeros(n)
    fro = f64()
    _check(lib().proxsdp_host_preprocess(C.byref(M.P), _p(order, pi64), _p(inv, pi64), _p(cs), C.byref(fro)))
    return order, inv, cs, fro.value


def host_equilibrate_rowsums(rowsums, n, options=None):
    """proxsdp_host_equilibrate_rowsums: (E, d) of equilibrate! from the row sums of squares of a Q x n matrix."""
    rs = _f(rowsums)
    E = np.zeros(max(len(rs), 1))
    d = f64()
    _check(lib().proxsdp_host_equilibrate_rowsums(_p(rs), len(rs), int(n), C.byref(options) if options is not None else None,
                                                  _p(E), C.byref(d)))
    return E[:len(rs)], d.value
