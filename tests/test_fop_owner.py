"""The owner form of the operator-form Lanczos step (kernels.hip.hpp fop_owner_body / k_lz_orth<., ., true>): one
workgroup per factor column finishes t = Vp'v inside the mat-vec launch, in the order in which every workgroup of k_lz_orth
adds the producers' records on the records form.  No sum changes, so a solve on the owner form IS the solve on the records
form (environment PROXSDP_HIP_FOP_OWNER = 0), bit for bit; stats["fop_owner_steps"] says which form the steps ran on."""
import numpy as np
import pytest

from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

pytestmark = pytest.mark.gpu

NOT_TIME = [c for c in range(14) if c != 12]       # trace column 12 is wall-clock time


def _both_forms(monkeypatch, n, iters, **kw):
    """(ref, sol): the same instance on the records form and with the switch unset, one process"""
    pr = P.maxcut(n, seed=0)
    kw = dict(max_iter=iters, support_path=1, lanczos_cycle_kernel=0, **kw)
    monkeypatch.setenv("PROXSDP_HIP_FOP_OWNER", "0")
    ref = Optimizer(**kw).optimize(pr, trace_capacity=iters)
    monkeypatch.delenv("PROXSDP_HIP_FOP_OWNER")
    sol = Optimizer(**kw).optimize(pr, trace_capacity=iters)
    print("n", n, "iterations", ref.iter, sol.iter, "restarts", ref.stats["lanczos_restarts"], sol.stats["lanczos_restarts"],
          "operator-form projections", ref.stats["fop_projections"], sol.stats["fop_projections"],
          "owner steps", ref.stats["fop_owner_steps"], sol.stats["fop_owner_steps"], "rank at the end", sol.trace[-1, 10])
    assert np.array_equal(sol.trace[:, NOT_TIME].view(np.uint64), ref.trace[:, NOT_TIME].view(np.uint64))
    assert np.array_equal(sol.primal, ref.primal) and np.array_equal(sol.dual_eq, ref.dual_eq)
    assert sol.status == ref.status and sol.iter == ref.iter
    assert sol.stats["lanczos_restarts"] == ref.stats["lanczos_restarts"]
    assert ref.stats["fop_projections"] > 0 and sol.stats["fop_projections"] > 0
    assert ref.stats["fop_owner_steps"] == 0
    return ref, sol


def test_one_or_two_columns_per_owner_with_restarts(monkeypatch):
    """n = 400: 7 workgroups, factor ranks up to 12 (owners of one column and of two), Krylov dimension 25 with restarts"""
    ref, sol = _both_forms(monkeypatch, 400, 60, initial_target_rank=12, max_target_rank_krylov_eigs=16)
    assert sol.stats["fop_owner_steps"] > 0 and sol.stats["lanczos_restarts"] > 0


def test_last_row_block_of_one_row(monkeypatch):
    """n = 257: 5 row blocks, the last one holds a single row; blocks 5 .. 63 are the +0.0 terms of the tree"""
    ref, sol = _both_forms(monkeypatch, 257, 40, initial_target_rank=8)
    assert sol.stats["fop_owner_steps"] > 0


def test_two_column_chunks_and_three_basis_chunks(monkeypatch):
    """n = 2100: 33 workgroups, factor ranks up to 66 = 2 nt (NCHP = 2: every owner holds two columns), basis chunks up to 3"""
    ref, sol = _both_forms(monkeypatch, 2100, 8, initial_target_rank=66, max_target_rank_krylov_eigs=70)
    assert sol.stats["fop_owner_steps"] > 0


def test_more_columns_than_two_per_workgroup_stay_on_the_records(monkeypatch):
    """n = 130 at rank 8: 3 workgroups, a factor rank above 6 has no owner for every column -- the records form, not by accident"""
    ref, sol = _both_forms(monkeypatch, 130, 30, initial_target_rank=8)
    assert sol.stats["fop_owner_steps"] == 0
