"""Host-side mirror of the reference's `ProxSDP.Optimizer` surface
(/root/reference/src/MOI_wrapper.jl) for the one path this build replaces.

MathOptInterface itself is Julia and is not re-implemented: a `Problem`
(problems.py) stands for the `OptimizerCache` that `MOI.copy_to` fills, and
`optimize()` is `_optimize!` (:220-342) with `chambolle_pock` (:310) replaced by
the C-ABI call.  Names, argument meaning and error behaviour follow the
reference so the parity tests read like its own tests:

    Optimizer(**kwargs)                  :69-81   unknown keyword -> error
    set_attribute / get_attribute        :84-103  RawOptimizerAttribute
    set_silent / silent                  :105-123 MOI.Silent
    set_time_limit_sec / time_limit_sec  :125-139 MOI.TimeLimitSec (None <-> 3600_00.0)
    termination_status ... dual_status   :377-441
    objective_value / dual_objective_value / solve_time_sec / pdhg_iterations
    variable_primal / constraint_* getters :451-530
"""
from . import binding

TERMINATION = {0: "OPTIMIZE_NOT_CALLED", 1: "OPTIMAL", 2: "TIME_LIMIT", 3: "ITERATION_LIMIT",
               4: "INFEASIBLE_OR_UNBOUNDED", 5: "DUAL_INFEASIBLE", 6: "INFEASIBLE"}


class Optimizer:
    SOLVER_NAME = "ProxSDP"            # MOI.SolverName, :77
    SOLVER_VERSION = "1.8.4"           # MOI.SolverVersion, :79 (the reference version mirrored)

    def __init__(self, **kwargs):
        self.options = binding.default_options()
        self.sol = None
        self.problem = None
        self.model = None                  # binding.Model kept by optimize(..., keep_model=True)
        for k, v in kwargs.items():
            self.set_attribute(k, v)

    # -- RawOptimizerAttribute
    def set_attribute(self, name, value):
        binding.set_option(self.options, name, float(value))
        return value

    def get_attribute(self, name):
        return binding.get_option(self.options, name)

    # -- MOI.Silent
    def set_silent(self, value):
        if value:
            self.options.timer_verbose = 0
        self.options.log_verbose = 0 if value else 1

    def silent(self):
        return not (self.options.log_verbose or self.options.timer_verbose)

    # -- MOI.TimeLimitSec
    def set_time_limit_sec(self, value):
        self.options.time_limit = 360000.0 if value is None else float(value)

    def time_limit_sec(self):
        v = self.options.time_limit
        return None if v == 360000.0 else v

    def is_empty(self):
        return self.problem is None and self.sol is None

    def empty(self):
        self.problem, self.sol = None, None

    # -- _optimize!
    def optimize(self, problem, eig_resid=None, trace_capacity=0, reduce=None, coupling=None, index_base=0,
                 nccl_comm=None, resume=None, capture_iteration=None, shards=None, device_ids=None, owners=None,
                 soc_owners=None, free_owners=None, factors=False, start=None, device_out=False, keep_model=False):
        """start: warm start (binding.solve: proxsdp_hip_solve_from) -- a dict (primal, dual_eq, dual_in, factors,
        target_rank, primal_step, beta; all in the units of a result) or a previous result of this optimizer; combines with
        factors=, not with shards=k, the state seam or a shard.
        factors=True | {cone: cap}: the low-rank factors of the PSD solution come back with the result
        (binding.solve: proxsdp_hip_solve_factored; `sol.psd_factors`, constraint_primal_psd_factor); not with shards=k.
        shards=k: the block-sharded solve from one call (binding.solve_sharded_inprocess) -- the library splits the model
        into k shards and runs them as host threads of this process, shard s on device_ids[s] (default: all on
        options.device_id); the result is the whole model's, the per-shard stats are kept in `self.shard_stats`.
        device_out=True: the result's vectors are float64 torch tensors on the solve's device (binding.solve:
        proxsdp_hip_solve_device), and the getters return what the result holds; start= then also takes CUDA tensors or a
        device result.  Not with shards=k, the state seam or a shard.
        keep_model=True: the solve runs on a binding.Model that stays on this optimizer (`self.model`), set up on the
        device; reoptimize() then replaces data of the same shape and solves again without that set-up.  The result is the
        one optimize() returns without the keyword.  Not with shards=k, the state seam or a shard."""
        self.empty()
        self.problem = problem
        self.shard_stats = None
        if self.model is not None:                         # (a kept model belongs to the problem it was built for)
            self.model.close()
            self.model = None
        if keep_model:
            if (shards is not None or reduce is not None or coupling is not None or nccl_comm or resume is not None or
                    capture_iteration is not None):
                raise ValueError("keep_model=True: the model must be whole, and there is no state seam")
            self.model = binding.Model(problem, self.options, eig_resid=eig_resid, index_base=index_base)
            sol = self.model.solve(start=start, factors=factors, device_out=device_out, trace_capacity=trace_capacity)
        elif shards is not None:
            if reduce is not None or coupling is not None or nccl_comm or resume is not None or capture_iteration is not None:
                raise ValueError("shards=...: the model must be whole (no reduce / coupling / nccl_comm) and there is no state seam")
            if factors is not False and factors is not None:
                raise ValueError("shards=...: the block-sharded solve does not return factors")
            if start is not None:
                raise ValueError("shards=...: the block-sharded solve has no warm start")
            if device_out:
                raise ValueError("shards=...: the block-sharded solve returns host arrays")
            sol, self.shard_stats = binding.solve_sharded_inprocess(
                problem, shards, device_ids=device_ids, owners=owners, soc_owners=soc_owners, free_owners=free_owners,
                options=self.options, trace_capacity=trace_capacity, eig_resid=eig_resid, index_base=index_base)
        else:
            sol = binding.solve(problem, self.options, eig_resid=eig_resid, trace_capacity=trace_capacity,
                                reduce=reduce, coupling=coupling, index_base=index_base, nccl_comm=nccl_comm,
                                resume=resume, capture_iteration=capture_iteration, factors=factors, start=start,
                                device_out=device_out)
        sign = -1.0 if problem.max_sense else 1.0          # :336-337
        sol.objval = sign * sol.objval + problem.objective_constant
        sol.dual_objval = sign * sol.dual_objval + problem.objective_constant
        self.sol = sol
        return sol

    def reoptimize(self, c=None, b=None, h=None, A_values=None, G_values=None, start=None, factors=False, device_out=False,
                   trace_capacity=0, add_rows=None, drop_rows=None):
        """After optimize(..., keep_model=True): replace data of the same shape (binding.Model.update: c, b, h as
        problem.c / .b / .h hold them -- c in the minimisation form, already sign-flipped for a max_sense problem --,
        A_values / G_values = the stored entries in sorted CSC order) and solve again on the kept model.  The sign and
        constant fix-up of optimize() applies: a max_sense problem keeps its sign.
        add_rows = (G_new, h_new) / drop_rows = row numbers: inequality rows added and dropped first
        (binding.Model.change_rows), before any value update; the optimizer's own problem (self.problem.G, .h) follows, so
        the getters and a later reoptimize(h=...) see the new shape; a start= that is a previous result of the old shape is
        carried over (its dual_in re-indexed, zeros on the new rows)."""
        if getattr(self, "model", None) is None:
            raise ValueError("reoptimize() needs optimize(..., keep_model=True) first")
        if add_rows is not None or drop_rows is not None:
            m_old = self.problem.G.shape[0]
            ch = self.model.change_rows(add=add_rows, drop=drop_rows)
            self._follow_rows(ch, add_rows)
            # a previous result can only be of the old shape; a dictionary is carried when its dual_in says so
            if isinstance(start, binding.SolveResult):
                start = ch.carry(start)
            elif start is not None and start.get("dual_in") is not None and len(start["dual_in"]) == m_old != ch.m:
                start = ch.carry(start)
        if any(v is not None for v in (c, b, h, A_values, G_values)):
            self.model.update(c=c, b=b, h=h, A_values=A_values, G_values=G_values)
        sol = self.model.solve(start=start, factors=factors, device_out=device_out, trace_capacity=trace_capacity)
        sign = -1.0 if self.problem.max_sense else 1.0
        sol.objval = sign * sol.objval + self.problem.objective_constant
        sol.dual_objval = sign * sol.dual_objval + self.problem.objective_constant
        self.sol = sol
        return sol

    def separate_triangles(self, result=None, **kw):
        """After optimize(..., keep_model=True): the most violated triangle inequalities of a PSD cone at `result` (default:
        the last solution) -- binding.Model.separate_triangles.  reoptimize(add_rows=cuts.add) appends them."""
        if getattr(self, "model", None) is None:
            raise ValueError("separate_triangles() needs optimize(..., keep_model=True) first")
        return self.model.separate_triangles(self.sol if result is None else result, **kw)

    def separate_cliques(self, result=None, bases=None, **kw):
        """After optimize(..., keep_model=True): the bases (a TriangleCuts, a CliqueCuts of size 5 or (nodes, signs)) grown
        into pentagonal / heptagonal rows at `result` (default: the last solution) -- binding.Model.separate_cliques.
        reoptimize(add_rows=cuts.add) appends them."""
        if getattr(self, "model", None) is None:
            raise ValueError("separate_cliques() needs optimize(..., keep_model=True) first")
        if bases is None:
            raise ValueError("separate_cliques() needs bases")
        return self.model.separate_cliques(self.sol if result is None else result, bases, **kw)

    def inactive_rows(self, result=None, **kw):
        """After optimize(..., keep_model=True): the inequality rows that went slack at `result` (default: the last
        solution) -- binding.Model.inactive_rows; a drop_rows list for reoptimize()."""
        if getattr(self, "model", None) is None:
            raise ValueError("inactive_rows() needs optimize(..., keep_model=True) first")
        return self.model.inactive_rows(self.sol if result is None else result, **kw)

    def round(self, result=None, **kw):
        """After optimize(..., keep_model=True, factors=...): a +-1 vector from the factors of `result` (default: the last
        solution) and the kept model's current objective -- binding.Model.round.  Its .objective is
        problem.user_objective(value) when the cone holds every variable of the model, None otherwise."""
        if getattr(self, "model", None) is None:
            raise ValueError("round() needs optimize(..., keep_model=True) first")
        out = self.model.round(self.sol if result is None else result, **kw)
        if len(self.problem.psd[kw.get("cone", 0)]) == self.problem.n:
            out.objective = self.problem.user_objective(out.value)
        self.last_round = out
        return out

    def bound(self, result=None, trace_cap=None):
        """After optimize(..., keep_model=True): a certified bound of the optimum from the duals of `result` (default: the
        last solution) -- binding.Model.bound, a device Cholesky test, no eigenvalue estimate.  Returns the DualBound; its
        .objective is the bound in the model's own sense, with the sign flip and the objective constant optimize() applies
        to objval: a LOWER bound of a minimisation, an UPPER bound of a max_sense problem."""
        if getattr(self, "model", None) is None:
            raise ValueError("bound() needs optimize(..., keep_model=True) first")
        out = self.model.bound(self.sol if result is None else result, trace_cap=trace_cap)
        out.objective = self.problem.user_objective(out.bound)
        self.last_bound = out
        return out

    def gap(self):
        """(bound, value of the last round()) in the model's own sense, when both exist (else None): the optimum lies
        between the two"""
        b, r = getattr(self, "last_bound", None), getattr(self, "last_round", None)
        if b is None or r is None or r.objective is None:
            return None
        return b.objective, r.objective

    def _follow_rows(self, ch, add_rows):
        """self.problem with the rows of the kept model: G' = [kept rows; new rows], h' likewise (host copies)"""
        import dataclasses
        import numpy as np
        import scipy.sparse as sp
        pr = self.problem
        k_old = ch.kept[ch.kept >= 0]
        G = sp.csr_matrix(pr.G, dtype=np.float64)[k_old, :]
        hh = np.asarray(pr.h, dtype=np.float64)[k_old]
        if add_rows is not None:
            _, ptr, cols, vals, h_new = binding._rows_arguments(add_rows, None, pr.n)
            to_np = lambda v: v.detach().cpu().numpy() if binding._is_tensor(v) else np.asarray(v, dtype=np.float64)
            Gn = sp.csr_matrix((to_np(vals).ravel(), cols, ptr), shape=(len(ptr) - 1, pr.n))
            G = sp.vstack([G, Gn], format="csr")
            hh = np.concatenate([hh, to_np(h_new).ravel()])
        self.problem = dataclasses.replace(pr, G=sp.csc_matrix(G), h=hh)

    # -- attributes set by optimize
    def termination_status(self):
        return TERMINATION[0 if self.sol is None else self.sol.status]

    def raw_status_string(self):
        return "Problem not solved" if self.sol is None else self.sol.status_string

    def primal_status(self, result_index=1):
        s = 0 if self.sol is None else self.sol.status
        if result_index > 1 or s == 0:
            return "NO_SOLUTION"
        if s == 5 and self.sol.certificate_found:
            return "INFEASIBILITY_CERTIFICATE"
        return "FEASIBLE_POINT" if self.sol.primal_feasible_user_tol else "INFEASIBLE_POINT"

    def dual_status(self, result_index=1):
        s = 0 if self.sol is None else self.sol.status
        if result_index > 1 or s == 0:
            return "NO_SOLUTION"
        if s == 6 and self.sol.certificate_found:
            return "INFEASIBILITY_CERTIFICATE"
        return "FEASIBLE_POINT" if self.sol.dual_feasible_user_tol else "INFEASIBLE_POINT"

    def result_count(self):
        return 0 if self.sol is None else self.sol.result_count

    def objective_value(self):
        return self.sol.objval

    def dual_objective_value(self):
        return self.sol.dual_objval

    def solve_time_sec(self):
        return self.sol.time

    def pdhg_iterations(self):
        return int(self.sol.iter)

    def variable_primal(self, idx=None):
        return self.sol.primal if idx is None else self.sol.primal[idx]

    def constraint_primal_psd(self, k):
        return self.sol.primal[self.problem.psd[k]]

    def constraint_primal_psd_factor(self, k):
        """(values, vectors, info) of PSD cone k: X_k ~ vectors diag(values) vectors' (optimize(..., factors=...))"""
        f = getattr(self.sol, "psd_factors", None)
        if f is None:
            raise RuntimeError("no factors: call optimize(..., factors=True) or factors={cone: cap}")
        return f[k]

    def constraint_dual_psd(self, k):
        return self.sol.dual_cone[self.problem.psd[k]]

    def constraint_primal_zeros(self):
        return self.sol.slack_eq

    def constraint_primal_nonpositives(self):
        return self.sol.slack_in

    def constraint_dual_zeros(self):
        return -self.sol.dual_eq            # :495-503

    def constraint_dual_nonpositives(self):
        return -self.sol.dual_in            # :505-513
