"""The model handle on the GPU (csrc/model.hip.hpp, csrc/model_update.hip.hpp, binding.Model): a solve on a handle IS the fresh
proxsdp_hip_solve_device call on the handle's current data -- whatever ran on the handle before, after host and device
updates, after a support rebuild, after a failed call.  "Equal" below is np.array_equal / == on: the six vectors, the trace
without its wall-clock column, iter, status, final_rank, the objectives, the gap, the residuals, the factors and every
integer counter of stats.  Long solves are capped with max_iter: an ITERATION_LIMIT result compares just as well."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

import kat_problems as K
import solve_request_cases as Q

pytestmark = pytest.mark.gpu

VECTORS = ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in")
SCALARS = ("status", "certificate_found", "primal_feasible_user_tol", "dual_feasible_user_tol", "result_count", "final_rank",
           "iter", "primal_residual", "dual_residual", "objval", "dual_objval", "gap", "dual_feasibility", "status_string")
INT_STATS = tuple(k for k, t in B.Stats._fields_ if t is B.i64) + ("reserved_s",)
TRACE_ELAPSED = 12
CAP = 48                                              # trace rows kept per solve
E_INVALID, E_UNSUPP = -1, -4


def _opts(**kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def _host(v):
    return v.cpu().numpy() if hasattr(v, "is_cuda") else np.asarray(v)


def _assert_equal(got, want, what):
    for k in SCALARS:
        a, b = getattr(got, k), getattr(want, k)
        assert a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b)), (what, k, a, b)
    for k in INT_STATS:
        assert got.stats[k] == want.stats[k], (what, k, got.stats[k], want.stats[k])
    keep = [c for c in range(B.TRACE_COLS) if c != TRACE_ELAPSED]
    assert got.trace.shape == want.trace.shape, (what, got.trace.shape, want.trace.shape)
    assert np.array_equal(got.trace[:, keep], want.trace[:, keep]), (what, "trace")
    for k in VECTORS:
        a, b = _host(getattr(got, k)), _host(getattr(want, k))
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()), float(np.abs(a - b).max(initial=0.0)))
    fa, fb = getattr(got, "psd_factors", None), getattr(want, "psd_factors", None)
    assert (fa is None) == (fb is None), what
    for (v1, V1, i1), (v2, V2, i2) in zip(fa or [], fb or []):
        assert np.array_equal(v1, v2) and np.array_equal(V1, V2) and i1 == i2, (what, "factors", i1, i2)


def _fresh(pr, okw, **skw):
    """the solve a handle must reproduce: proxsdp_hip_solve_device through binding.solve"""
    return B.solve(pr, _opts(**okw), trace_capacity=CAP, device_out=True, factors=True, **skw)


def _on_model(mdl, **skw):
    return mdl.solve(trace_capacity=CAP, device_out=True, factors=True, **skw)


def _assert_dumps_equal(a, b, what, norms_equal=True):
    for k, _ in B.MODEL_DUMP_ARRAYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("n", "Q", "nnz", "ns"):
        assert a[k] == b[k], (what, k)
    if norms_equal:
        for k in B.MODEL_NORM_NAMES:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _with(pr, **kw):
    """a copy of `pr` with some members replaced"""
    d = dict(n=pr.n, A=pr.A, b=pr.b, G=pr.G, h=pr.h, c=pr.c, psd=pr.psd, soc=pr.soc, max_sense=pr.max_sense,
             objective_constant=pr.objective_constant)
    d.update(kw)
    return P.Problem(**d)


def _stored(M):
    M = sp.csc_matrix(M, dtype=np.float64)
    M.sort_indices()
    return M


# the side-96 Max-Cut of most tests: n = 4656, degree 6, the Krylov branch from side 33 on -- the support path (auto: n >= 4096
# and a support of 96 + 288 entries), the operator-form mat-vec and the one-workgroup cycle kernel
SIDE96 = dict(min_size_krylov_eigs=32, max_iter=40)


def _maxcut96(seed=0):
    return P.maxcut(96, seed=seed, avg_degree=6.0)


# ----------------------------------------------------------------- 1. repeat
def _two_blocks():
    return P.block_diag_problems([_maxcut96(0), _maxcut96(1)])


REPEAT = {
    # name: (problem, options, the counters that show the path the row names)
    "side12_small_block_batch": (lambda: P.maxcut(12, seed=0), dict(max_iter=60), ("batched_small_eigs",)),
    "side96_support_operator_cycle": (_maxcut96, SIDE96, ("fop_projections", "cycle_launches")),
    "side96_sign_projection": (_maxcut96, dict(full_eig_decomp=1, max_iter=25), ("full_eigs_sign",)),
    "side96_dsyevd": (_maxcut96, dict(full_eig_decomp=1, full_eig_sign=0, max_iter=15), ("full_eigs",)),
    "side288_rank32_split_merge": (lambda: P.maxcut(288, seed=0, avg_degree=6.0),
                                   dict(initial_target_rank=32, max_target_rank_krylov_eigs=40, max_iter=12),
                                   ("lanczos_matvecs", "device_eig_merges")),
    "two_blocks_batched_lanczos": (_two_blocks, dict(min_size_krylov_eigs=32, support_path=0, max_iter=30),
                                   ("batched_block_steps",)),
    "mixed_cones_soc_1x1_free": (K.mixed_cones, dict(max_iter=120), ("lanczos_matvecs",)),
    "infeasible_lp_certificate": (K.infeasible_lp, dict(max_iter=2000, max_obj=10.0, certificate_search=1), ()),
    "unbounded_lp_certificate": (K.unbounded_lp, dict(max_obj=1e300, certificate_search=1), ()),
    "infeasible_sdp_certificate_support": (K.infeasible_sdp, dict(support_path=1), ("fop_projections",)),
}


@pytest.mark.parametrize("name", sorted(REPEAT))
def test_three_solves_on_one_handle_each_equal_the_fresh_solve(name):
    make, okw, counters = REPEAT[name]
    pr = make()
    want = _fresh(pr, okw)
    print(name, "status", want.status, "iter", want.iter, {k: want.stats[k] for k in counters})
    for k in counters:
        assert want.stats[k] > 0, (name, k, "the case no longer takes the path it is here for")
    if name == "side96_dsyevd":
        assert want.stats["full_eigs_sign"] == 0
    if name.endswith("certificate") or "certificate" in name:
        assert want.certificate_found, "the case no longer runs a certificate search to its end"
    reps = 2 if name.startswith("infeasible_sdp") else 3           # (3500 iterations a solve: the second one is the test)
    with B.Model(pr, _opts(**okw)) as mdl:
        for k in range(reps):
            _assert_equal(_on_model(mdl), want, (name, "solve", k))
        assert mdl.info()["solves"] == reps


# ----------------------------------------------------------------- 2. order independence
def test_warm_cold_and_device_start_on_one_handle_equal_their_fresh_calls():
    pr = _maxcut96()
    first = _fresh(pr, SIDE96)
    warm = _fresh(pr, SIDE96, start=first)
    host_start = dict(B.start_from_result(first))
    dev_start = dict(host_start)                                  # primal and duals stay CUDA tensors: start_dev
    host_start.update(primal=_host(first.primal), dual_eq=_host(first.dual_eq), dual_in=_host(first.dual_in))
    warm_host = _fresh(pr, SIDE96, start=host_start)
    with B.Model(pr, _opts(**SIDE96)) as mdl:
        _assert_equal(_on_model(mdl), first, "first")
        _assert_equal(_on_model(mdl, start=host_start), warm_host, "warm from host arrays")
        _assert_equal(_on_model(mdl), first, "cold after warm")
        _assert_equal(_on_model(mdl, start=dev_start), warm, "warm from device tensors")
        _assert_equal(_on_model(mdl), first, "cold again")


def test_two_handles_alive_at_once_solved_alternately():
    pa, pb = _maxcut96(0), P.maxcut(12, seed=3)
    oa, ob = SIDE96, dict(max_iter=50)
    wa, wb = _fresh(pa, oa), _fresh(pb, ob)
    with B.Model(pa, _opts(**oa)) as ma, B.Model(pb, _opts(**ob)) as mb:
        for k in range(2):
            _assert_equal(_on_model(ma), wa, ("a", k))
            _assert_equal(_on_model(mb), wb, ("b", k))


# ----------------------------------------------------------------- 3. update, host route
def _perturbed_c(pr, seed=5):
    """every edge weight (every nonzero of c) changed by a seeded +-1 %: the zero pattern stays"""
    rng = np.random.default_rng(seed)
    return pr.c * (1.0 + 0.01 * rng.choice([-1.0, 1.0], size=len(pr.c)))


def test_host_update_of_c_and_b_equals_a_fresh_model_of_the_updated_problem():
    pr = _maxcut96()
    c2, b2 = _perturbed_c(pr), pr.b * 1.25
    pr2 = _with(pr, c=c2, b=b2)
    old = _fresh(pr, SIDE96)
    want = _fresh(pr2, SIDE96, start=old)
    with B.Model(pr, _opts(**SIDE96)) as mdl, B.Model(pr2, _opts(**SIDE96)) as ref:
        _assert_equal(_on_model(mdl), old, "before the update")
        mdl.update(c=c2, b=b2)
        _assert_dumps_equal(mdl.dump(), ref.dump(), "c and b")
        _assert_equal(_on_model(mdl, start=old), want, "after the update")
        info = mdl.info()
        assert info["support_rebuilds"] == 0 and info["updates"] == 1 and info["use_support"] == 1


def test_host_update_of_h_and_G_values_on_the_mixed_model():
    pr = K.mixed_cones()
    okw = dict(max_iter=120)
    rng = np.random.default_rng(11)
    G2 = _stored(pr.G)
    G2.data = G2.data * (1.0 + 0.01 * rng.choice([-1.0, 1.0], size=len(G2.data)))
    h2 = pr.h + 0.05
    pr2 = _with(pr, G=G2, h=h2)
    old = _fresh(pr, okw)
    want = _fresh(pr2, okw, start=old)
    with B.Model(pr, _opts(**okw)) as mdl, B.Model(pr2, _opts(**okw)) as ref:
        mdl.update(h=h2, G_values=G2.data)
        _assert_dumps_equal(mdl.dump(), ref.dump(), "h and G")
        _assert_equal(_on_model(mdl, start=old), want, "after the update")
        assert mdl.info()["support_rebuilds"] == 0


# ----------------------------------------------------------------- 4. pattern change
def test_a_changed_zero_pattern_of_c_rebuilds_the_support_once():
    pr = _maxcut96()
    c2 = pr.c.copy()
    A = _stored(pr.A)
    empty = np.diff(A.indptr) == 0
    enters = int(np.flatnonzero(empty & (c2 == 0.0))[7])           # a zero of c in an empty column: joins the support
    leaves = int(np.flatnonzero(empty & (c2 != 0.0))[3])           # a nonzero of c in an empty column: leaves it
    c2[enters], c2[leaves] = 1.0, 0.0
    pr2 = _with(pr, c=c2)
    first, want = _fresh(pr, SIDE96), _fresh(pr2, SIDE96)
    with B.Model(pr, _opts(**SIDE96)) as mdl, B.Model(pr2, _opts(**SIDE96)) as ref:
        _assert_equal(_on_model(mdl), first, "before")
        mdl.update(c=c2)
        assert mdl.info()["support_rebuilds"] == 1
        got, exp = mdl.dump(), ref.dump()
        assert got["ns"] > 0 and np.array_equal(got["support"], exp["support"])
        _assert_dumps_equal(got, exp, "after the pattern change")
        _assert_equal(_on_model(mdl), want, "after the pattern change")
        mdl.update(c=pr.c)
        assert mdl.info()["support_rebuilds"] == 2
        _assert_equal(_on_model(mdl), first, "back to the first data")


# ----------------------------------------------------------------- 5. update, device route
def test_norm2_kernel_gives_the_same_bits_at_every_launch_width():
    v = np.random.default_rng(2).standard_normal(3 * 4096 + 123)
    vals = {g: B.model_norm2(v, grid=g) for g in (0, 1, 3, 37)}
    assert len(set(vals.values())) == 1, vals
    assert abs(vals[0] - np.linalg.norm(v)) <= 4 * np.finfo(float).eps * np.sqrt(len(v)) * np.linalg.norm(v)
    assert B.model_norm2(np.array([3.0, 4.0])) == 5.0


def test_device_update_of_integer_data_equals_the_host_update():
    """Integer-valued data -- weights in 1 .. 8, integer b, integer diagonal entries of A (columns with the factor 1) -- make
    every square an integer <= 64 and every sum of squares an integer below 64 * 4656 < 2^19, far below 2^53: exact in any
    order, so the device route's norms must equal the host's and with them the whole solve."""
    import torch
    pr = _maxcut96()
    rng = np.random.default_rng(9)
    c2 = np.where(pr.c != 0.0, rng.integers(1, 9, size=len(pr.c)).astype(float), 0.0)
    b2 = rng.integers(1, 4, size=len(pr.b)).astype(float)
    a2 = rng.integers(1, 3, size=_stored(pr.A).nnz).astype(float)
    cuda = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    with B.Model(pr, _opts(**SIDE96)) as mh, B.Model(pr, _opts(**SIDE96)) as md:
        mh.update(c=c2, b=b2, A_values=a2)
        md.update(c=cuda(c2), b=cuda(b2), A_values=cuda(a2))
        _assert_dumps_equal(md.dump(), mh.dump(), "integer data")
        _assert_equal(_on_model(md), _on_model(mh), "integer data")
        assert md.info()["support_rebuilds"] == 0


def test_device_update_of_float_data_agrees_in_the_norms_and_equals_elsewhere():
    """4 eps sqrt(len) relative: a random-walk estimate of the rounding of a sum of len squares, not its worst case"""
    import torch
    pr = _maxcut96()
    c2, b2 = _perturbed_c(pr, seed=6), pr.b * 1.1
    cuda = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    with B.Model(pr, _opts(**SIDE96)) as mh, B.Model(pr, _opts(**SIDE96)) as md:
        mh.update(c=c2, b=b2)
        md.update(c=cuda(c2), b=cuda(b2))
        dh, dd = mh.dump(), md.dump()
        _assert_dumps_equal(dd, dh, "float data", norms_equal=False)
        lens = dict(norm_b=len(pr.b), norm_h=max(len(pr.h), 1), norm_c=len(pr.c), frob=dh["nnz"])
        for k in B.MODEL_NORM_NAMES:
            print(k, dh[k], dd[k], abs(dh[k] - dd[k]) / max(dh[k], 1e-300))
            assert abs(dh[k] - dd[k]) <= 4 * np.finfo(float).eps * np.sqrt(lens[k]) * abs(dh[k]), k


# ----------------------------------------------------------------- 6. failure leaves the handle whole
def test_failed_calls_leave_the_handle_whole():
    import torch
    pr = _maxcut96()
    want = _fresh(pr, SIDE96)
    with B.Model(pr, _opts(**SIDE96)) as mdl:
        _assert_equal(_on_model(mdl), want, "first")
        bad = torch.zeros(pr.n, dtype=torch.float64, device="cuda:0")
        bad[5] = float("nan")
        with pytest.raises(B.ProxSDPHipError) as e:
            _on_model(mdl, start=dict(primal=bad))
        assert e.value.code == E_INVALID and "primal" in str(e.value)
        _assert_equal(_on_model(mdl), want, "after a non-finite device start")
        before = mdl.dump()
        c_bad = pr.c.copy()
        c_bad[3] = np.inf
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.update(c=c_bad)
        assert e.value.code == E_INVALID
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.update(b=torch.tensor(np.full(len(pr.b), np.nan), dtype=torch.float64, device="cuda:0"))
        assert e.value.code == E_INVALID and "b" in str(e.value)
        _assert_dumps_equal(mdl.dump(), before, "after refused updates")
        assert mdl.info()["updates"] == 0
        _assert_equal(_on_model(mdl), want, "after refused updates")
        cut = _on_model(mdl, time_limit=1e-9)
        assert cut.status == 2 and cut.iter < want.iter, (cut.status, cut.iter)
        _assert_equal(_on_model(mdl), want, "after a time limit")


# ----------------------------------------------------------------- 7. refusals on the device
def test_run_options_may_change_the_limits_and_nothing_else():
    pr = _maxcut96()
    with B.Model(pr, _opts(**SIDE96)) as mdl:
        o = _opts(**SIDE96)
        B.set_option(o, "tol_gap", 1e-3)
        R = B.Result()
        rc = B.lib().proxsdp_hip_model_solve(mdl._h, C.byref(o), C.byref(R), None, None, None, None)
        assert rc == E_INVALID and "tol_gap" in B.lib().proxsdp_hip_last_error().decode()
        want17 = _fresh(pr, dict(SIDE96, max_iter=17))
        _assert_equal(_on_model(mdl, max_iter=17), want17, "max_iter = 17")
        _assert_equal(_on_model(mdl), _fresh(pr, SIDE96), "the model's own limit again")


def test_an_equilibrated_model_takes_no_update_and_repeats_its_solves():
    pr = K.sdp_wiki(False)
    okw = dict(equilibration_force=1)
    want = _fresh(pr, okw)
    with B.Model(pr, _opts(**okw)) as mdl:
        _assert_equal(_on_model(mdl), want, 0)
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.update(c=pr.c)
        assert e.value.code == E_UNSUPP
        _assert_equal(_on_model(mdl), want, 1)
        _assert_equal(_on_model(mdl), want, 2)


def test_a_value_update_needs_the_approximate_norm():
    pr = K.sdp_wiki(False)
    okw = dict(approx_norm=0)
    want = _fresh(pr, okw)
    with B.Model(pr, _opts(**okw)) as mdl:
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.update(A_values=_stored(pr.A).data)
        assert e.value.code == E_UNSUPP
        _assert_equal(_on_model(mdl), want, "approx_norm = 0")
        mdl.update(c=pr.c * 2.0)                                      # (c does not enter sigma_max)
        _assert_equal(_on_model(mdl), _fresh(_with(pr, c=pr.c * 2.0), okw), "approx_norm = 0, new c")


def test_a_handle_refuses_a_damaged_request_as_solve_device_does():
    """every case of the start table and of the device-vector table (solve_request_cases; the shard cases do not apply: a
    handle has no shard fields) against proxsdp_hip_model_solve: refused on the host -- the fake device pointers of the table
    are never read -- with the code and the message proxsdp_hip_solve_device gives for the same damage; no solve is counted,
    and the handle then solves as a fresh call does"""
    pr = K.sdp_wiki(False)
    want = _fresh(pr, {})
    with B.Model(pr, _opts()) as mdl:
        for table, cases in (("start", Q.START_CASES), ("device", Q.DEVICE_CASES)):
            for case in cases:
                rc, msg = Q.request_call("model_solve", table, case, handle=mdl._h)
                rc_dev, msg_dev = Q.request_call("solve_device", table, case)
                assert rc == E_INVALID and rc_dev == E_INVALID, (table, case, rc, rc_dev, msg, msg_dev)
                assert msg and msg == msg_dev, (table, case, msg, msg_dev)
        assert mdl.info()["solves"] == 0
        _assert_equal(_on_model(mdl), want, "after the refused requests")
        assert mdl.info()["solves"] == 1


# ----------------------------------------------------------------- 8. the Python surface
def _assert_same_sol(a, b, what):
    for k in ("status", "iter", "objval", "dual_objval", "gap", "final_rank"):
        assert getattr(a, k) == getattr(b, k), (what, k, getattr(a, k), getattr(b, k))
    for k in VECTORS:
        assert np.array_equal(_host(getattr(a, k)), _host(getattr(b, k))), (what, k)


@pytest.mark.parametrize("max_sense", [False, True])
def test_reoptimize_equals_optimize_of_the_updated_problem(max_sense):
    pr = _with(_maxcut96(), max_sense=max_sense, objective_constant=3.5)
    c2 = _perturbed_c(pr)
    pr2 = _with(pr, c=c2)
    kept = Optimizer(**SIDE96)
    s0 = kept.optimize(pr, keep_model=True, factors=True)
    plain = Optimizer(**SIDE96)
    p0 = plain.optimize(pr, factors=True)
    _assert_same_sol(s0, p0, "optimize(keep_model=True)")
    start = B.start_from_result(p0)
    s1 = kept.reoptimize(c=c2, start=start)
    p1 = Optimizer(**SIDE96).optimize(pr2, start=start)
    _assert_same_sol(s1, p1, "reoptimize")
    assert kept.objective_value() == p1.objval
    sign = -1.0 if max_sense else 1.0
    raw = B.solve(pr2, _opts(**SIDE96), start=start)
    assert s1.objval == sign * raw.objval + 3.5
    kept.model.close()


def test_a_closed_model_frees_its_device_memory():
    pr = _maxcut96()
    with B.Model(pr, _opts(**SIDE96)) as mdl:
        first = mdl.info()["device_bytes"]
        assert first > 8 * pr.n
        _on_model(mdl)
        assert mdl.info()["device_bytes"] >= first
    with pytest.raises(ValueError):
        mdl.info()
    with B.Model(pr, _opts(**SIDE96)) as again:
        assert again.info()["device_bytes"] == first
