"""Block-sharded solve from ONE call (proxsdp_hip_solve_sharded): the library splits the whole model, runs one shard per
host thread of this process and returns the whole model's result in the caller's order.  All shards run on device 0 (the
test box has one GPU); the contract against the single-process solve is the one of tests/test_sharded_mixed.py::_contract
and tests/test_sharded_gpu.py: same status and iteration count, the same linesearch trials in every iteration, trace
columns 1, 2, 7 to rtol 1e-9 / atol 1e-12, objectives to 1e-9 relative, final_rank equal, the whole-model primal to 1e-9."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from kat_problems import mixed_cones
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------- models (those of the per-process sharded tests)
def _two_maxcut():
    return P.block_diag_problems([P.maxcut(120, seed=1), P.maxcut(150, seed=2)], name="two-maxcut")


def _couple(pr, d00, d11):
    """X1[0,0] + 2 X2[0,0] = 3 and X1[1,1] - X2[1,1] <= 0.5 (variables 0 and 2 are entries (0,0) and (1,1) of the first
    block's triangle, d00 and d11 those of the other block): rows no shard owns alone"""
    import scipy.sparse as sp
    row = sp.csr_matrix(([1.0, 2.0], ([0, 0], [0, d00])), shape=(1, pr.n))
    g = sp.csr_matrix(([1.0, -1.0], ([0, 0], [2, d11])), shape=(1, pr.n))
    return P.Problem(n=pr.n, A=sp.vstack([pr.A, row]).tocsc(), b=np.append(pr.b, 3.0),
                     G=sp.vstack([pr.G, g]).tocsc(), h=np.append(pr.h, 0.5), c=pr.c, psd=pr.psd, soc=pr.soc,
                     name=pr.name + "-coupled")


def _model(key):
    """(model, shards, owners, soc_owners, free_owners, options of the single-process reference)"""
    if key == "two-maxcut":
        return _two_maxcut(), 2, None, None, None, dict(support_path=1)
    if key == "two-maxcut-coupled":
        n1 = P.maxcut(120, seed=1).n
        return _couple(_two_maxcut(), n1, n1 + 2), 2, None, None, None, dict(support_path=1)
    if key == "mixed":
        return mixed_cones(0), 2, None, None, None, {}
    if key == "mixed-first-cone-on-1":                   # the model's first PSD cone (side 1) on shard 1: trace column 10 is that shard's
        return mixed_cones(0), 2, [1, 0, 1, 0, 0], [0], None, {}
    if key == "mixed3":                                   # shard 2 holds only the SOC and the free variables
        return mixed_cones(0), 3, [0, 1, 0, 1, 1], [2], [2, 2, 2], {}
    if key == "paths":                                    # shard 0: the Max-Cut block alone (support path); shard 1: the rest
        mc, mx = P.maxcut(120, seed=1), mixed_cones(2)
        big = mx.psd[2]
        pr = _couple(P.block_diag_problems([mc, mx], name="maxcut-mixed"), mc.n + big[0], mc.n + big[2])
        return pr, 2, [0] + [1] * len(mx.psd), [1], [1] * 3, {}
    raise KeyError(key)


_REF = {}


def _reference(key):
    """the single-process solve, computed once per model (the mixed cases share one model, whatever their owners)"""
    pr, _, _, _, _, kw = _model(key)
    key = "mixed" if key.startswith("mixed") else key
    if key not in _REF:
        _REF[key] = Optimizer(max_iter=300, **kw).optimize(pr, trace_capacity=300)
    return _REF[key]


# ----------------------------------------------------------------- the kernel: coupling rows across shards
def _coupling_case(S, L, seed):
    """order-revealing partials (1e16, 1, -1e16, ... dealt over the shards), -0.0 in every shard at some rows, and a
    scattered, non-monotone row list with an odd first row into a longer vector"""
    rng = np.random.default_rng(seed)
    big = np.array([1e16, 1.0, -1e16, 3.0, 1.0, 1.0, -1.0, 1e16])
    parts = rng.standard_normal((S, L))
    for k in range(0, L, 3):
        parts[:, k] = np.roll(big, k)[:S]
    parts[:, 1::7] = -0.0
    n = 2 * L + 7
    rows = rng.permutation(np.arange(1, n, 2))[:L]            # odd rows only (an odd first row with them), shuffled
    v = rng.standard_normal(n)
    return parts, rows, v


@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_coupling_sum_kernel_adds_in_shard_order_and_scatters(S):
    assert B.device_count() > 0
    for L in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025):     # around the workgroup size (256), one and several workgroups
        parts, rows, v = _coupling_case(S, L, 100 * S + L)
        acc = parts[0].copy()
        for r in range(1, S):
            acc += parts[r]
        exp = v.copy()
        exp[rows] = acc
        got = B.coupling_sum(parts, rows, v)
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), (S, L)       # bits: -0.0 stays -0.0
        assert L < 2 or np.signbit(got[rows[1]])
        untouched = np.setdiff1d(np.arange(len(v)), rows)
        assert np.array_equal(got[untouched], v[untouched])
    with pytest.raises(B.ProxSDPHipError):
        B.coupling_sum(np.zeros((2, 3)), [0, 1, 9], np.zeros(9))                      # a row outside the vector


# ----------------------------------------------------------------- one shard = the plain solve
def test_one_in_process_shard_is_the_plain_solve_bit_for_bit():
    assert B.device_count() > 0
    pr = mixed_cones(0)
    ref = _reference("mixed")
    opt = Optimizer(max_iter=300)
    sol = opt.optimize(pr, trace_capacity=300, shards=1)
    assert sol.iter == ref.iter and sol.status == ref.status
    assert np.array_equal(sol.primal, ref.primal)
    cols = [c for c in range(ref.trace.shape[1]) if c != 12]            # 12: elapsed seconds
    assert sol.trace.shape == ref.trace.shape and np.array_equal(sol.trace[:, cols], ref.trace[:, cols])
    assert len(opt.shard_stats) == 1 and opt.shard_stats[0]["sharded_general_iterations"] == sol.iter
    assert sol.stats["lanczos_matvecs"] == opt.shard_stats[0]["lanczos_matvecs"]


# ----------------------------------------------------------------- several shards = the plain solve
def _contract(pr, ref, sol):
    assert sol.status == ref.status and sol.iter == ref.iter, (sol.status, ref.status, sol.iter, ref.iter)
    assert np.array_equal(sol.trace[:, 11], ref.trace[:, 11])                       # same linesearch trials
    R = ref.trace[:, [1, 2, 7]]
    excess = np.abs(sol.trace[:, [1, 2, 7]] - R) / (1e-12 + 1e-9 * np.abs(R))
    print("trace columns 1, 2, 7: largest |difference| / (atol + rtol |ref|) = %.3g at iteration %d"
          % (excess.max(), 1 + int(np.argmax(excess.max(axis=1)))))
    assert np.allclose(sol.trace[:, [1, 2, 7]], R, rtol=1e-9, atol=1e-12)
    assert abs(sol.objval - ref.objval) <= 1e-9 * (1 + abs(ref.objval))
    assert abs(sol.dual_objval - ref.dual_objval) <= 1e-9 * (1 + abs(ref.dual_objval))
    assert sol.final_rank == ref.final_rank
    print("largest |primal - single process| = %.3g" % np.abs(sol.primal - ref.primal).max())
    assert np.allclose(sol.primal, ref.primal, rtol=0, atol=1e-9)


@pytest.mark.parametrize("key", ["two-maxcut", "two-maxcut-coupled", "mixed", "mixed-first-cone-on-1", "mixed3", "paths"])
def test_in_process_shards_reproduce_the_single_process_solve(key):
    assert B.device_count() > 0
    pr, shards, owners, soc_owners, free_owners, _ = _model(key)
    ref = _reference(key)
    opt = Optimizer(max_iter=300)
    sol = opt.optimize(pr, trace_capacity=300, shards=shards, device_ids=[0] * shards, owners=owners,
                       soc_owners=soc_owners, free_owners=free_owners)
    _contract(pr, ref, sol)
    st = opt.shard_stats
    assert len(st) == shards
    # the whole model's counters are the shards' sums; the mat-vec column of the trace is summed the same way
    assert sol.stats["lanczos_matvecs"] == sum(s["lanczos_matvecs"] for s in st)
    # (every mat-vec of a projection is counted in its iteration's column 13 and in lanczos_matvecs alike; the trace holds
    # every iteration; so the column of the whole model adds up to the total of ALL shards -- one shard's column would not)
    print("mat-vecs per iteration equal to the single-process solve's:", bool(np.array_equal(sol.trace[:, 13], ref.trace[:, 13])))
    assert sol.trace[:, 13].sum() == sum(s["lanczos_matvecs"] for s in st) > 0
    if key.startswith("two-maxcut"):
        assert min(s["lanczos_matvecs"] for s in st) > 0      # both shards contribute to the column
    assert np.array_equal(sol.trace[:, 10], ref.trace[:, 10])      # target rank of the model's first PSD cone
    general = [s["sharded_general_iterations"] for s in st]
    if key.startswith("two-maxcut"):
        assert general == [0, 0]                              # both shards on the support path
    elif key == "paths":
        assert general == [0, sol.iter] and st[0]["fop_projections"] + st[0]["lanczos_matvecs"] > 0
    elif key == "mixed3":
        assert general[2] == sol.iter and st[2]["lanczos_matvecs"] == 0       # no PSD block there
    else:
        assert sol.iter in general


def test_start_vectors_are_split_per_cone():
    """eig_resid (one start vector per PSD cone, in the caller's cone order) with shards=: every shard gets the vectors of
    ITS cones.  The owners interleave the cones (1, 0, 1, 0, 0), so a walk that handed a shard the first vectors of the list
    would give its blocks vectors of the wrong cones.  Reference: the single-process solve with the same vectors; a solve
    with other vectors takes other Lanczos steps, which the mat-vec column shows."""
    assert B.device_count() > 0
    pr = mixed_cones(0)
    rng = np.random.default_rng(5)
    # a start vector far from the default one: almost all weight on one coordinate, another coordinate per cone
    er = []
    for k, side in enumerate(pr.psd_sides()):
        v = 1e-3 * rng.standard_normal(side)
        v[(3 * k) % side] += 1.0
        er.append(v)
    ref = Optimizer(max_iter=300).optimize(pr, trace_capacity=300, eig_resid=er)
    opt = Optimizer(max_iter=300)
    sol = opt.optimize(pr, trace_capacity=300, shards=2, owners=[1, 0, 1, 0, 0], soc_owners=[0], eig_resid=er)
    _contract(pr, ref, sol)
    print("mat-vecs per iteration: with the vectors", ref.trace[:3, 13], "in-process", sol.trace[:3, 13],
          "default vectors", _reference("mixed").trace[:3, 13], "whole column equal:",
          bool(np.array_equal(sol.trace[:, 13], ref.trace[:, 13])))
    # iteration 1 projects the start point (one step whatever the vector); iteration 2 holds the first Lanczos runs proper,
    # started from the caller's vectors, on matrices that agree between the paths to the last ulps after ONE iteration: their
    # step count is the single-process solve's with these vectors, and (what makes this a test of the split) not the count
    # the default vectors give
    assert ref.trace[1, 13] != _reference("mixed").trace[1, 13], "the start vectors of this test do not show in iteration 2"
    assert sol.trace[1, 13] == ref.trace[1, 13]


# ----------------------------------------------------------------- to the optimum, in user order
def test_to_the_optimum_in_the_callers_order():
    assert B.device_count() > 0
    pr = mixed_cones(0)
    ref = Optimizer().optimize(pr, trace_capacity=2000)
    assert ref.status == 1
    sol = Optimizer().optimize(pr, trace_capacity=2000, shards=2)
    print("iterations", sol.iter, "single process", ref.iter, "per iteration: %.1f us in-process shards, %.1f us single"
          % (1e6 * sol.trace[-1, 12] / sol.iter, 1e6 * ref.trace[-1, 12] / ref.iter))
    assert sol.status == 1
    assert abs(sol.iter - ref.iter) <= max(3, 0.05 * ref.iter)
    assert abs(sol.objval - ref.objval) <= 2e-6 * (1 + abs(ref.objval))
    assert sol.final_rank == ref.final_rank
    sc = max(1.0, np.abs(ref.primal).max())
    for k in ("primal", "slack_eq", "slack_in", "dual_eq", "dual_in"):
        assert np.allclose(getattr(sol, k), getattr(ref, k), rtol=0, atol=2e-5 * sc), k
    for idx, side in zip(pr.psd, pr.psd_sides()):
        assert np.linalg.eigvalsh(P.unpack_psd(sol.primal[idx], side)).min() >= -1e-6
    t = sol.primal[pr.soc[0]]
    assert t[0] >= np.linalg.norm(t[1:]) - 1e-6


# ----------------------------------------------------------------- restrictions keep their codes
def test_restrictions_of_a_sharded_solve_keep_their_codes():
    pr = mixed_cones(0)
    for kw, code in ((dict(approx_norm=0), -4), (dict(equilibration=1), -4), (dict(equilibration_force=1), -4)):
        with pytest.raises(B.ProxSDPHipError) as e:
            Optimizer(max_iter=5, **kw).optimize(pr, shards=2)
        assert e.value.code == code, kw
    with pytest.raises(B.ProxSDPHipError) as e:
        Optimizer(max_iter=5).optimize(pr, shards=2, device_ids=[0, 4096])
    assert e.value.code == -1
    with pytest.raises(B.ProxSDPHipError) as e:                      # the fault switch needs its environment variable
        Optimizer(max_iter=5, debug_fail_iteration=3).optimize(pr, shards=2)
    assert e.value.code == -1 and "PROXSDP_HIP_FAULT_INJECTION" in str(e.value)


def test_the_model_must_be_whole():
    """nccl_comm / reduce_vec_fn / reduce_fn on the model handed to the one-call solve, or a dense A (M_dense):
    PROXSDP_E_INVALID before any thread starts (the pointers are never used: a non-NULL value is all the check looks at)"""
    pr = mixed_cones(0)
    cb = B.REDUCE_FN(lambda ctx, ps, ns, pm, nm: 0)
    cbv = B.REDUCE_VEC_FN(lambda ctx, ptr, length, on_device: 0)
    o = B.default_options()
    o.max_iter = 5
    for field, value in (("nccl_comm", B.C.c_void_p(8)), ("reduce_vec_fn", B.C.cast(cbv, B.C.c_void_p)),
                         ("reduce_fn", B.C.cast(cb, B.C.c_void_p)), ("M_dense", B.C.c_void_p(8))):
        M = B._Marshalled(pr, None, 0)
        setattr(M.P, field, value)
        arrays = [np.zeros(max(k, 1)) for k in (M.P.n, M.P.n, M.P.p, M.P.m, M.P.p, M.P.m)]
        R = B.Result()
        R.primal, R.dual_cone, R.dual_eq, R.dual_in, R.slack_eq, R.slack_in = [B._p(a) for a in arrays]
        rc = B.lib().proxsdp_hip_solve_sharded(B.C.byref(M.P), B.C.byref(o), 2, None, None, None, None, B.C.byref(R), None)
        assert rc == -1, (field, rc)
        with pytest.raises(B.ProxSDPHipError, match="A_dense cannot" if field == "M_dense" else "must not itself be a shard"):
            B._check(rc)


# ----------------------------------------------------------------- a failing shard ends the call
def _failing_child(q, inject):
    if inject:
        os.environ["PROXSDP_HIP_FAULT_INJECTION"] = "1"
    pr = mixed_cones(0)
    kw = dict(debug_fail_iteration=7) if inject else {}
    try:
        sol = Optimizer(max_iter=300, **kw).optimize(pr, shards=2)
        q.put(("solved", int(sol.status), int(sol.iter)))
    except B.ProxSDPHipError as e:
        q.put(("error", e.code, str(e)))


def _run_child(inject):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_failing_child, args=(q, inject))
    p.start()
    try:
        out = q.get(timeout=120)                             # a hang shows up as queue.Empty here
        p.join(timeout=60)
    finally:
        if p.is_alive():                                     # a child that hangs must not stay behind with the GPU open
            p.kill()
            p.join()
    assert p.exitcode == 0
    return out


def test_a_failing_shard_ends_the_call_with_its_error():
    """debug_fail_iteration = 7 throws a C++ exception on the host inside the LAST shard's projection of iteration 7 (no GPU
    fault is involved): that shard still joins the iteration's reduce, every shard stops after it, and the call returns the
    failing shard's code and text in the caller's thread.  Afterwards a fresh process solves the same model."""
    kind, code, msg = _run_child(True)
    assert kind == "error", (kind, code, msg)
    assert code == -5 and "shard 1 of 2" in msg and "injected projection failure" in msg, msg
    assert "[shards stopped in iteration 7 7]" in msg, msg
    kind, status, it = _run_child(False)
    assert kind == "solved" and it == _reference("mixed").iter


# ----------------------------------------------------------------- two devices
def test_two_shards_on_two_devices():
    if B.device_count() < 2:
        pytest.skip("needs 2 GPUs: the peer-access reads of the coupling-row kernel; device 0 alone covers the same kernel "
                    "and barrier in test_in_process_shards_reproduce_the_single_process_solve")
    pr, shards, owners, soc_owners, free_owners, _ = _model("two-maxcut-coupled")
    sol = Optimizer(max_iter=300).optimize(pr, trace_capacity=300, shards=2, device_ids=[0, 1])
    _contract(pr, _reference("two-maxcut-coupled"), sol)
