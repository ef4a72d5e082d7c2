"""The device merge inside solves (options.device_eig_merge): golden traces at Krylov dimension 25, auto mode at Krylov
dimension 65 against the host merge, and a merge the device path does not serve."""
import json

import numpy as np
import pytest

from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

from test_gpu_parity import _assert_trace_rows

pytestmark = pytest.mark.gpu

NOT_TIME = [c for c in range(14) if c != 12]       # trace column 12 is wall-clock time


@pytest.mark.parametrize("name", ["sdplib_mcp124-1", "maxcut_er_n200_s0"])
def test_golden_traces_with_the_merge_on_the_device(name, golden_dir):
    """test_iteration_traces_match_golden's rows and criteria with host_eig_merge = 1 and device_eig_merge = 1: every
    K x K eigensolve of these runs (Krylov dimension 25) is split, and its merge runs on the device"""
    gold = json.loads((golden_dir / "traces.json").read_text())[name]
    if name == "sdplib_mcp124-1":
        pr, iters = P.sdplib(golden_dir / "sdplib" / "mcp124-1.dat-s"), 120
    else:
        pr, iters = P.maxcut(200, seed=0), 120
    opt = Optimizer(max_iter=iters, host_eig_merge=1, device_eig_merge=1)
    sol = opt.optimize(pr, trace_capacity=iters)
    rows = np.array(gold["rows"])
    assert sol.status == gold["status"] and sol.iter == gold["iter"]
    assert sol.stats["device_eig_merges"] > 0 and sol.stats["host_eig_merges"] >= sol.stats["device_eig_merges"]
    print(name, "device merges", sol.stats["device_eig_merges"], "fallbacks", sol.stats["device_eig_merge_fallbacks"])
    k = min(len(rows), len(sol.trace))
    assert k == len(rows)
    deg = gold["degenerate_iters"]
    upto = (deg[0] - 1) if deg else k                 # rows before the first degenerate projection
    assert [it for it in gold["restart_iters"] if it <= upto], "the tight window must include Lanczos restarts"
    assert upto >= 50
    _assert_trace_rows(sol.trace, rows, upto, name)
    if not deg:
        assert abs(opt.objective_value() - gold["objval"]) <= 1e-9 * (1 + abs(gold["objval"]))


def test_auto_mode_at_krylov_dimension_65_follows_the_host_merge():
    """Max-Cut n = 400 at target rank 32: Krylov dimension 65, the step kernels, the split path -- auto mode sends the merges
    to the device.  The run with the merge on the host is the reference: same discrete history, objectives to 1e-9,
    residual-type columns to 1e-7 (the suite's trace tolerances)."""
    pr = P.maxcut(400, seed=0)
    kw = dict(max_iter=40, initial_target_rank=32, max_target_rank_krylov_eigs=64)
    ref = Optimizer(device_eig_merge=0, **kw).optimize(pr, trace_capacity=40)
    sol = Optimizer(device_eig_merge=-1, **kw).optimize(pr, trace_capacity=40)
    print("host", ref.status, ref.iter, ref.stats["host_eig_merges"], ref.stats["lanczos_restarts"],
          "| device", sol.stats["device_eig_merges"], sol.stats["device_eig_merge_fallbacks"], sol.stats["lanczos_restarts"])
    assert ref.stats["device_eig_merges"] == 0 and ref.stats["device_eig_merge_fallbacks"] == 0
    assert ref.stats["host_eig_merges"] > 0 and ref.stats["lanczos_restarts"] > 0
    assert sol.stats["device_eig_merges"] > 0 and sol.stats["device_eig_merge_fallbacks"] == 0
    assert sol.stats["device_eig_merges"] == sol.stats["host_eig_merges"] == ref.stats["host_eig_merges"]
    assert sol.stats["lanczos_restarts"] == ref.stats["lanczos_restarts"] > 0
    assert sol.status == ref.status and sol.iter == ref.iter == 40
    assert np.array_equal(sol.trace[:, 13], ref.trace[:, 13])                   # Lanczos mat-vecs per iteration
    _assert_trace_rows(sol.trace, ref.trace, 40, "device against host merge")   # iter, ranks, trials equal; 1e-9 / 1e-7
    assert abs(sol.objval - ref.objval) <= 1e-9 * (1 + abs(ref.objval))
    # the device merge returns the host merge's bits, so the two solves are the same solve
    assert np.array_equal(sol.trace[:, NOT_TIME], ref.trace[:, NOT_TIME])


def test_a_merge_the_device_does_not_serve_is_done_by_the_host():
    """Two PSD blocks of different sides are projected by block worker threads, which keep the host merge: with the
    device path switched on every merge is a counted fallback and the solve is the host-merge solve, bit for bit."""
    pr = P.block_diag_problems([P.maxcut(150, seed=0), P.maxcut(170, seed=1)])
    kw = dict(max_iter=30, host_eig_merge=1, block_batch=0)
    ref = Optimizer(device_eig_merge=0, **kw).optimize(pr, trace_capacity=30)
    sol = Optimizer(device_eig_merge=1, **kw).optimize(pr, trace_capacity=30)
    print("fallbacks", sol.stats["device_eig_merge_fallbacks"], "host merges", sol.stats["host_eig_merges"])
    assert ref.stats["host_eig_merges"] > 0 and ref.stats["device_eig_merge_fallbacks"] == 0
    assert sol.stats["device_eig_merges"] == 0
    assert sol.stats["device_eig_merge_fallbacks"] == sol.stats["host_eig_merges"] == ref.stats["host_eig_merges"]
    assert sol.status == ref.status and sol.iter == ref.iter
    assert np.array_equal(sol.trace[:, NOT_TIME], ref.trace[:, NOT_TIME])
    assert np.array_equal(sol.primal, ref.primal)
