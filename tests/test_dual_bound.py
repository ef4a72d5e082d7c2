"""The certified dual bound on the device (proxsdp_hip_model_bound, proxsdp_hip_cholesky; include/proxsdp_hip.h "a certified
dual bound").  Fixtures and the NumPy side of the checks: tests/bound_cases.py.

- the factorisation kernels alone (proxsdp_hip_cholesky): the exact integer cases bit for bit and against the host's flag,
  the cases that must fail, the backward-error inequality the certificate assumes on seeded real matrices, two runs alike
- Model.bound on the known-optimum cases: bound <= p*, the tightness rule against the ideal bound of the same duals, host
  and device duals alike, derived and explicit caps alike, a solve before and after the call bit-identical
- end to end on Max-Cut n = 60 through two triangle rounds"""
import numpy as np
import pytest
import torch

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

import bound_cases as K
pytestmark = pytest.mark.gpu

VECTORS = ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in")
SCALARS = ("status", "iter", "primal_residual", "dual_residual", "objval", "dual_objval", "gap", "dual_feasibility")


def _opts(**kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def _host(v):
    return v.cpu().numpy() if hasattr(v, "is_cuda") else np.asarray(v)


# ---------------------------------------------------------------------------------------------- the factorisation kernels
@pytest.mark.parametrize("side", K.FACTOR_SIDES)
def test_integer_products_factor_exactly_and_agree_with_the_host(side):
    for kind in ("unit", "scaled"):
        L = K.integer_factor(side, 0, kind)
        A = K.product(L)
        fail, R = B.cholesky(A)
        hfail, hR = B.host_cholesky(A)
        assert fail == hfail == -1, (side, kind, fail, hfail)
        assert np.array_equal(R, L.T) and np.array_equal(hR, L.T), (side, kind)
        fail2, R2 = B.cholesky(A)
        assert fail2 == fail and np.array_equal(R2, R), (side, kind, "two runs")
        # a shift that keeps everything an integer square: A + 3 I is not L L', so only the flag is exact here
        assert B.cholesky(A, shift=3.0, want_factor=False)[0] == -1


@pytest.mark.parametrize("side", K.FACTOR_SIDES)
def test_the_product_minus_eps_fails_where_it_is_proved_indefinite(side):
    A, eps = K.minus_eps(K.product(K.integer_factor(side, 0, "unit")))
    fail, _ = B.cholesky(A, want_factor=False)
    if side <= 2:                                                    # (positive definite: bound_cases.py says why)
        assert np.linalg.eigvalsh(A).min() > 0.1 and fail == -1
        return
    assert K.indefinite_witness(K.product(K.integer_factor(side, 0, "unit"))), side
    assert 0 <= fail < side, (side, fail)
    assert B.cholesky(A, want_factor=False)[0] == fail, "two runs"
    assert B.host_cholesky(A, want_factor=False)[0] >= 0


@pytest.mark.parametrize("side", K.FACTOR_SIDES)
def test_a_bad_pivot_in_the_last_column_a_zero_matrix_and_one_by_one(side):
    A, L = K.last_pivot_bad(side, 1)
    fail, R = B.cholesky(A)
    assert fail == B.host_cholesky(A, want_factor=False)[0] == side - 1, (side, fail)
    assert np.array_equal(R[:side - 1, :], L.T[:side - 1, :]), "the columns before the failure hold L"
    zero = np.zeros((side, side))
    assert B.cholesky(zero, want_factor=False)[0] == B.host_cholesky(zero, want_factor=False)[0] == 0
    assert B.cholesky(np.full((side, side), np.nan), want_factor=False)[0] == 0        # a NaN pivot is a result
    if side == 1:
        fail, R = B.cholesky(np.array([[9.0]]))
        assert fail == -1 and R.tolist() == [[3.0]]
        assert B.cholesky(np.array([[-9.0]]), want_factor=False)[0] == 0
        assert B.cholesky(np.array([[-9.0]]), shift=25.0)[1].tolist() == [[4.0]]


@pytest.mark.parametrize("side", K.FACTOR_SIDES)
def test_the_backward_error_bound_the_certificate_assumes(side):
    A = K.spd_real(side, 0)
    fail, R = B.cholesky(A)
    assert fail == -1 and np.all(np.tril(R, -1) == 0.0)
    K.assert_backward_error(A, R, f"side {side}")
    fail2, R2 = B.cholesky(A)
    assert fail2 == -1 and np.array_equal(R2, R), "two runs give identical bits"
    hfail, hR = B.host_cholesky(A)
    assert hfail == -1
    K.assert_backward_error(A, hR, f"side {side} (host)")


def test_the_test_entry_refuses_what_it_does_not_serve():
    L = B.lib()
    fail = B.C.c_int64(7)
    one = np.ones(1)
    assert L.proxsdp_hip_cholesky(None, 1, 0.0, None, B.C.byref(fail)) == -1
    assert L.proxsdp_hip_cholesky(B._p(one), 0, 0.0, None, B.C.byref(fail)) == -1
    assert L.proxsdp_hip_cholesky(B._p(one), 1, -1.0, None, B.C.byref(fail)) == -1
    assert L.proxsdp_hip_cholesky(B._p(one), 1, float("nan"), None, B.C.byref(fail)) == -1
    assert L.proxsdp_hip_cholesky(B._p(one), 1, 0.0, None, None) == -1
    assert fail.value == 7


# ---------------------------------------------------------------------------------------------- Model.bound, known optimum
@pytest.mark.parametrize("side", K.BOUND_SIDES_GPU)
def test_known_optimum_bound_tightness_routes_caps_and_an_untouched_handle(side):
    case = K.known_optimum(side)
    pr, p_star = case["problem"], case["p_star"]
    none = np.zeros(0)
    with B.Model(pr, _opts(max_iter=40)) as mdl:
        before = mdl.solve()
        for kind in ("exact", "uniform", "seeded"):
            ye, Zt, lam = K.duals(case, kind)
            db = mdl.bound((ye, none))
            what = f"side {side}, {kind} duals"
            assert db.certified.all() and db.bound <= p_star, (what, db.bound, p_star)      # exact comparison
            assert db.dual_objective == -float(ye.sum()), what                              # dyadic numbers: an exact sum
            K.assert_tight(db, 0, Zt, what)
            assert db.trace[0] >= side and db.trace[0] <= side * (1 + 1e-12)
            assert 1 <= db.factorisations[0] <= 19 and db.bytes_allocated >= 2 * 8 * side * side
            # the ideal bound of these duals, and how far the certificate is from it
            ideal = -float(ye.sum()) + side * min(0.0, float(np.linalg.eigvalsh(Zt).min()))
            assert db.bound >= ideal - 1.01 * db.loss - 1e-9 * (1.0 + np.abs(ye).sum()), (what, db.bound, ideal, db.loss)
            if lam is not None:
                assert ideal == pytest.approx(p_star, abs=1e-4)
            # device duals: the same bits
            dev = mdl.bound((torch.tensor(ye, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda")))
            for k in ("shift", "lambda_lower", "radius", "delta", "trace", "factorisations"):
                assert np.array_equal(getattr(dev, k), getattr(db, k)), (what, k)
            assert dev.bound == db.bound and dev.dual_objective == db.dual_objective, what
            # explicit caps equal to the derived ones: the same bits
            cap = mdl.bound((ye, none), trace_cap=db.trace)
            assert cap.bound == db.bound and np.array_equal(cap.lambda_lower, db.lambda_lower), what
            # a looser cap can only lower the bound
            assert mdl.bound((ye, none), trace_cap=[2.0 * side]).bound <= db.bound
        after = mdl.solve()
        for k in SCALARS:
            assert getattr(before, k) == getattr(after, k), k
        for k in VECTORS:
            assert np.array_equal(_host(getattr(before, k)), _host(getattr(after, k))), k
        info = mdl.info()
        # refusals leave the handle as it was
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.bound((np.full(side, np.nan), none))
        assert e.value.code == -1 and "dual_eq" in str(e.value)
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.bound((torch.full((side,), float("inf"), dtype=torch.float64, device="cuda"),
                       torch.zeros(0, dtype=torch.float64, device="cuda")))
        assert e.value.code == -1 and "dual_eq" in str(e.value)
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.bound((case["y"].astype(float), none), trace_cap=[-1.0])
        assert e.value.code == -1
        assert mdl.info()["device_bytes"] == info["device_bytes"]


def test_models_the_call_does_not_serve_are_refused_with_the_reason():
    pr = P.maxcut(20, seed=0)
    with B.Model(pr, _opts(equilibration=1, equilibration_force=1)) as mdl:
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.bound((np.zeros(mdl.p), np.zeros(mdl.m)))
        assert e.value.code == -4 and "equilibrated" in str(e.value)


# ---------------------------------------------------------------------------------------------- end to end
def test_maxcut_60_the_bound_follows_two_triangle_rounds():
    """P.maxcut(60, seed=0, avg_degree=6.0), the instance of tests/test_clique_cuts.py: solve, bound, two rounds of the 100
    most violated triangle rows with a warm re-solve and a bound after each.  Bounds are UPPER bounds of the MAX model.
    TOLERANCES.  The certificate's loss T (sigma* + delta + rho) is, up to the search's 10 %, T |lambda_min(Z~)| with T = 60:
    the dual infeasibility of the point handed in, which the solver's stopping rule does not bound.  The last assertion asks
    for a fall of the bound beyond both losses; two rounds of 100 rows lower the optimum of this instance by 3.7 (the CPU
    oracle's 144.867 -> 141.192, tests/test_clique_cuts.py), so the duals must put lambda_min well below 3.7 / 60 / 10 =
    6e-3.  Stopping tolerances of 1e-4 do not promise that (recorded on an MI355X with the default options: lambda_min
    -1.3e-3, -6.0e-3, -3.3e-2 and losses 0.083, 0.39, 2.09 for the three solves, bounds 144.921, 142.885, 142.869 -- every
    one valid and tight for its duals, the last fall of 2.05 short of 0.083 + 2.09); the solves here stop at 1e-6
    (recorded: lambda_min -2.2e-6, -9.5e-5, -3.1e-5, losses 1.4e-4, 6.1e-3, 1.9e-3, bounds 144.8616, 142.5964, 141.2580
    beside objval 144.8616, 142.5906, 141.2564; the best cut found is 139)."""
    pr = P.maxcut(60, seed=0, avg_degree=6.0)
    opt = Optimizer(tol_gap=1e-6, tol_feasibility=1e-6, tol_feasibility_dual=1e-6, tol_primal=1e-6, tol_dual=1e-6)
    with pytest.raises(ValueError):
        opt.bound()
    r = opt.optimize(pr, keep_model=True, factors=True)
    assert opt.gap() is None
    bounds, losses = [], []
    for rnd in range(3):
        if rnd:
            cuts = opt.separate_triangles(count=100, min_violation=0.02)
            assert len(cuts) > 0
            r = opt.reoptimize(add_rows=cuts.add, start=r, factors=True)
        assert r.status == 1
        db = opt.bound()
        cut = opt.round(trials=192, seed=1)
        Zt = K.dual_matrices(opt.problem, _host(r.dual_eq), _host(r.dual_in))[0]
        K.assert_tight(db, 0, Zt, f"maxcut 60, round {rnd}")
        assert db.objective == -db.bound and db.certified.all()
        assert opt.gap() == (db.objective, cut.objective)
        print(f"round {rnd}: objval {r.objval:.6f}, dual_objval {r.dual_objval:.6f}, certified bound {db.objective:.6f}, "
              f"loss {db.loss:.3g}, cut {cut.objective}")
        assert db.objective >= cut.objective, (rnd, db.objective, cut.objective)
        bounds.append(db.objective); losses.append(db.loss)
    assert bounds[2] < bounds[0] - (losses[0] + losses[2]), (bounds, losses)
    opt.model.close()
