"""The low-rank factors a solve hands back (proxsdp_hip_solve_factored through binding.solve(..., factors=...)).

Everything is recomputed with numpy from what the call returned: Xk is the block unpacked from res.primal, (values,
vectors) the factors of that cone, u = 2^-53.  Bounds:

RITZ (the last projection's Ritz pairs; the block IS their reconstruction):
    resid <= 8 (r + 4) u trace(Xk).  The reconstruction and the residual kernel both evaluate sum_k lam_k v_ik v_jk with
    relative error <= gamma_{r+1} on sum_k lam_k |v_ik| |v_jk|; the Frobenius norm of that matrix is <= sum lam = trace;
    the sqrt(2) round trip of the off-diagonals adds 2 u: 2 (r + 4) u trace, with a factor 4 of slack.
EIG (one dsyevd of the final block, lambda > 0 kept):
    resid <= 16 max(||Xk - (Xk)+||_F by numpy's eigh on the same matrix, n u ||Xk||_F): LAPACK on the same input is the
    measure, the factor 16 covers rocSOLVER against LAPACK.
reported resid / xnorm against numpy's: 64 u xnorm (two Frobenius sums in different orders).
eigenvalues (Weyl): |lam_lib - lam_numpy| <= resid + ||V'V - I||_2 lam_max + n u lam_max, every term from the output.
orthonormality of RITZ vectors is what the Lanczos run left, not derivable: it is compared with the CPU oracle's Ritz
    vectors of the same block, <= 100 max(oracle's, n u)."""
import numpy as np
import pytest

import oracle
from oracle import eig as oeig
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import moi
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

from kat_problems import mixed_cones, sdp_wiki

U = 2.0 ** -53
TRACE_ELAPSED = 12                                  # trace column 12 is wall-clock time: the one column two runs do not share


def options(**kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def block(x, pr, k):
    return P.unpack_psd(x[pr.psd[k]], B.psd_sides(pr)[k])


def fro_resid(Xk, vals, vecs):
    return float(np.linalg.norm(Xk - (vecs * vals) @ vecs.T))


def ritz_bound(Xk, r):
    return 8.0 * (r + 4) * U * float(np.trace(Xk))


def eig_bound(Xk):
    w, Q = np.linalg.eigh(Xk)
    pos = w > 0.0
    ref = float(np.linalg.norm(Xk - (Q[:, pos] * w[pos]) @ Q[:, pos].T))
    return 16.0 * max(ref, Xk.shape[0] * U * float(np.linalg.norm(Xk))), ref


def check_cone(name, Xk, fac, expect_source=None):
    """the assertions every cone of side >= 2 shares; returns (numpy's residual, the bound that applied)"""
    vals, vecs, info = fac
    n = Xk.shape[0]
    r = info["rank"]
    assert vals.shape == (r,) and vecs.shape == (n, r)
    assert info["rank"] == min(info["cap"], info["rank_found"])
    assert np.all(vals > 0.0) and np.all(np.diff(vals) <= 0.0), vals
    xn = float(np.linalg.norm(Xk))
    res_np = fro_resid(Xk, vals, vecs)
    src = info["source"]
    if src == B.FACTOR_RITZ:
        bound, ref = ritz_bound(Xk, info["rank_found"]), None
    else:
        bound, ref = eig_bound(Xk)
    print(f"{name}: side {n} source {info['source_name']} rank {r}/{info['rank_found']} resid lib {info['resid']:.3e} "
          f"numpy {res_np:.3e} bound {bound:.3e}" + (f" (numpy's own {ref:.3e}: ratio {info['resid'] / max(ref, 1e-300):.2f})" if ref is not None else "")
          + f" xnorm lib {info['xnorm']:.17g} numpy {xn:.17g}")
    if expect_source is not None:
        assert src == expect_source, (name, info["source_name"])
    assert abs(info["xnorm"] - xn) <= 64 * U * xn
    assert abs(info["resid"] - res_np) <= 64 * U * xn
    if info["rank"] == info["rank_found"]:
        assert info["resid"] <= bound, (name, info["resid"], bound)
    return res_np, bound


# ------------------------------------------------------------------------------------------------ Max-Cut n = 120, defaults
@pytest.fixture(scope="module")
def maxcut():
    pr = P.maxcut(120, seed=0)
    cap = 20000
    sol = B.solve(pr, options(), trace_capacity=cap, factors=True)
    assert sol.trace.shape[0] < cap
    return pr, sol


@pytest.mark.gpu
def test_maxcut_default_solve_returns_the_ritz_pairs(maxcut):
    pr, sol = maxcut
    assert sol.status == 1 and len(sol.psd_factors) == 1
    Xk = block(sol.primal, pr, 0)
    vals, vecs, info = sol.psd_factors[0]
    check_cone("maxcut120", Xk, sol.psd_factors[0], expect_source=B.FACTOR_RITZ)
    assert sum(f[2]["rank"] for f in sol.psd_factors) == sol.final_rank
    assert info["rank"] == info["rank_found"]
    assert info["resid"] <= ritz_bound(Xk, info["rank"])
    # the Optimizer's getter hands out the same triple
    opt = Optimizer()
    s2 = opt.optimize(pr, factors={0: 3})
    v3, V3, i3 = opt.constraint_primal_psd_factor(0)
    assert i3["rank"] == 3 and np.array_equal(v3, vals[:3]) and np.array_equal(V3, vecs[:, :3])
    assert np.array_equal(s2.primal, sol.primal)


@pytest.mark.gpu
def test_maxcut_eigenvalues_within_weyl(maxcut):
    pr, sol = maxcut
    Xk = block(sol.primal, pr, 0)
    vals, vecs, info = sol.psd_factors[0]
    r = info["rank"]
    w = np.linalg.eigvalsh(Xk)[::-1][:r]
    orth = float(np.linalg.norm(vecs.T @ vecs - np.eye(r), 2))
    bound = info["resid"] + orth * vals[0] + Xk.shape[0] * U * vals[0]
    print(f"eigenvalues: max |lib - numpy| {np.abs(vals - w).max():.3e}, bound {bound:.3e} (resid {info['resid']:.3e}, orth {orth:.3e})")
    assert np.abs(vals - w).max() <= bound


@pytest.mark.gpu
def test_maxcut_ritz_vectors_are_as_orthonormal_as_the_oracles(maxcut):
    pr, sol = maxcut
    Xk = block(sol.primal, pr, 0)
    vals, vecs, info = sol.psd_factors[0]
    n, r = Xk.shape[0], info["rank"]
    lib = float(np.linalg.norm(vecs.T @ vecs - np.eye(r), 2))
    o = oracle.Options()
    arc = oeig.EigSolverAlloc(n, o)
    oeig.krylovkit_eig(arc, np.asfortranarray(Xk), r, o)
    k = min(r, arc.converged_eigs)
    assert k >= 1
    Z = np.asarray(arc.vecs)[:, :k]
    ref = float(np.linalg.norm(Z.T @ Z - np.eye(k), 2))
    print(f"orthonormality ||V'V - I||_2: library {lib:.3e}, oracle {ref:.3e} ({k} pairs), n u {n * U:.3e}")
    assert lib <= 100.0 * max(ref, n * U)


@pytest.mark.gpu
def test_cap_one_returns_the_top_pair_and_reports_what_was_cut(maxcut):
    pr, full = maxcut
    sol = B.solve(pr, options(), factors={0: 1})
    assert np.array_equal(sol.primal, full.primal)
    Xk = block(sol.primal, pr, 0)
    vals, vecs, info = sol.psd_factors[0]
    assert info["rank"] == 1 and info["rank_found"] > 1 and info["rank_found"] == full.psd_factors[0][2]["rank_found"]
    assert info["source"] == B.FACTOR_RITZ
    w, Q = np.linalg.eigh(Xk)
    lam1, v1, lam2 = w[-1], Q[:, -1], w[-2]
    v = vecs[:, 0]
    # the pair is numpy's top pair: Weyl for the value, Davis-Kahan for the vector (residual of the pair over its gap)
    fi = full.psd_factors[0][2]
    fV = full.psd_factors[0][1]
    orth = float(np.linalg.norm(fV.T @ fV - np.eye(fV.shape[1]), 2))
    assert abs(vals[0] - lam1) <= fi["resid"] + orth * lam1 + Xk.shape[0] * U * lam1
    rv = float(np.linalg.norm(Xk @ v - vals[0] * v))
    vn = v / np.linalg.norm(v)
    sin = float(np.linalg.norm(vn - np.sign(vn @ v1) * v1))          # 2 sin(angle / 2): >= sin(angle), equal to first order
    print(f"cap=1: lam {vals[0]:.15g} numpy {lam1:.15g}, sin(angle) {sin:.3e}, pair residual {rv:.3e}, gap {lam1 - lam2:.3e}")
    assert sin <= 2.0 * rv / (lam1 - lam2) + 8 * Xk.shape[0] * U * lam1 / (lam1 - lam2)       # (second term: numpy's own v1)
    xn = float(np.linalg.norm(Xk))
    cut_np = float(np.linalg.norm(Xk - lam1 * np.outer(v1, v1)))
    print(f"cap=1: resid lib {info['resid']:.15g} numpy (its own top pair) {cut_np:.15g}")
    assert abs(info["resid"] - fro_resid(Xk, vals, vecs)) <= 64 * U * xn
    assert abs(info["resid"] - cut_np) <= 64 * U * xn + ritz_bound(Xk, info["rank_found"])


@pytest.mark.gpu
def test_iteration_limit_factors_still_describe_the_returned_primal():
    pr = P.maxcut(120, seed=0)
    sol = B.solve(pr, options(max_iter=3), factors=True)
    assert sol.status == 3 and sol.iter == 3
    check_cone("maxcut120 max_iter=3", block(sol.primal, pr, 0), sol.psd_factors[0])


# ------------------------------------------------------------------------------------------------ EIG sources
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["full_eig_decomp", "kat_3x3", "equilibration_force", "equilibration_force_intended",
                                  "kat_3x3_equilibrated"])
def test_blocks_that_are_not_ritz_reconstructions_get_one_eigendecomposition(name):
    """equilibration_force = 1 on the Max-Cut instance drives the iterate to X = 0 (the reference's aliased scaling iteration,
    equilibration_reference_aliasing = 1, is not contractive: the solve ends INFEASIBLE): the case is kept as it is, and
    the same instance under the intended iteration (aliasing = 0) and the equilibrated 3 x 3 KAT give it blocks that are
    not zero."""
    if name.startswith("kat_3x3"):
        pr, o = sdp_wiki(False), options(**({"equilibration_force": 1} if name.endswith("equilibrated") else {}))
    elif name == "equilibration_force_intended":
        pr, o = P.maxcut(120, seed=0), options(max_iter=400, equilibration_force=1, equilibration_reference_aliasing=0)
    else:
        pr, o = P.maxcut(120, seed=0), options(max_iter=400, **{name: 1})
    sol = B.solve(pr, o, factors=True)
    for k in range(len(pr.psd)):
        check_cone(f"{name} cone {k}", block(sol.primal, pr, k), sol.psd_factors[k], expect_source=B.FACTOR_EIG)
        assert sol.psd_factors[k][2]["rank"] == sol.psd_factors[k][2]["rank_found"]
        if name != "equilibration_force":
            assert sol.psd_factors[k][2]["xnorm"] > 0.0 and sol.psd_factors[k][2]["rank"] > 0


# ------------------------------------------------------------------------------------------------ mixed cones
MIXED_ITERS = 3000                                  # (the model reaches OPTIMAL after ~940 iterations)


@pytest.fixture(scope="module")
def mixed():
    pr = mixed_cones(1, sides=(5, 130, 1), soc_len=4, nfree=1)
    return pr, B.solve(pr, options(max_iter=MIXED_ITERS), factors=True)


@pytest.mark.gpu
def test_mixed_model_sources_are_per_cone_in_the_callers_order(mixed):
    pr, sol = mixed
    assert [f[1].shape[0] for f in sol.psd_factors] == [5, 130, 1]
    assert sol.status == 1
    srcs = [f[2]["source"] for f in sol.psd_factors]
    print("mixed sources:", [f[2]["source_name"] for f in sol.psd_factors], "ranks", [f[2]["rank"] for f in sol.psd_factors])
    assert srcs[0] == B.FACTOR_EIG and srcs[1] == B.FACTOR_RITZ and srcs[2] == B.FACTOR_NONE
    for k in (0, 1):
        check_cone(f"mixed cone {k}", block(sol.primal, pr, k), sol.psd_factors[k])
    vals, vecs, info = sol.psd_factors[2]
    x = float(sol.primal[pr.psd[2][0]])
    if x > 0.0:
        assert info["rank"] == 1 and vals.tolist() == [x] and vecs.tolist() == [[1.0]] and info["resid"] == 0.0
    else:
        assert info["rank"] == 0 and info["resid"] == abs(x)
    assert info["xnorm"] == abs(x)


@pytest.mark.gpu
def test_cap_zero_writes_nothing_for_that_cone(mixed):
    pr, full = mixed
    sol = B.solve(pr, options(max_iter=MIXED_ITERS), factors={1: 2})
    assert np.array_equal(sol.primal, full.primal)
    for k in (0, 2):
        vals, vecs, info = sol.psd_factors[k]
        assert info == dict(rank=0, rank_found=0, source=B.FACTOR_NONE, source_name="NONE", resid=0.0, xnorm=0.0, cap=0)
        assert vals.size == 0 and vecs.size == 0
    vals, vecs, info = sol.psd_factors[1]
    fv, fV, fi = full.psd_factors[1]
    assert info["rank"] == min(2, fi["rank_found"]) and info["rank_found"] == fi["rank_found"]
    assert np.array_equal(vals, fv[:info["rank"]]) and np.array_equal(vecs, fV[:, :info["rank"]])


# ------------------------------------------------------------------------------------------------ the solve is untouched
def same_solve(a, b, primal=True):
    assert a.status == b.status and a.iter == b.iter and a.final_rank == b.final_rank
    cols = [c for c in range(a.trace.shape[1]) if c != TRACE_ELAPSED]
    assert a.trace.shape == b.trace.shape and np.array_equal(a.trace[:, cols], b.trace[:, cols])
    for f in ("dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in") + (("primal",) if primal else ()):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.objval == b.objval and a.dual_objval == b.dual_objval and a.gap == b.gap
    for k in ("lanczos_matvecs", "lanczos_restarts", "full_eigs", "linesearch_trials", "exit_matvecs", "fop_projections"):
        assert a.stats[k] == b.stats[k], k


@pytest.mark.gpu
def test_the_factored_solve_is_the_plain_solve_bit_for_bit(maxcut, mixed):
    pr, fac = maxcut
    plain = B.solve(pr, options(), trace_capacity=20000)
    assert not hasattr(plain, "psd_factors")
    same_solve(fac, plain)
    nop = B.solve(pr, options(), trace_capacity=20000, factors=True, primal=False)      # res->primal = NULL
    assert nop.primal is None
    same_solve(nop, plain, primal=False)
    for (v0, V0, i0), (v1, V1, i1) in zip(fac.psd_factors, nop.psd_factors):
        assert np.array_equal(v0, v1) and np.array_equal(V0, V1) and i0 == i1
    prm, facm = mixed
    same_solve(facm, B.solve(prm, options(max_iter=MIXED_ITERS)))


@pytest.mark.gpu
def test_a_shard_is_refused_by_the_factored_entry_only():
    pr = P.maxcut(20, seed=3)
    with pytest.raises(B.ProxSDPHipError) as e:
        B.solve(pr, options(max_iter=5), factors=True, reduce=lambda sums, maxs: None)
    assert e.value.code == -4
    assert B.solve(pr, options(max_iter=5), reduce=lambda sums, maxs: None).iter == 5    # the plain entry still serves it


# ------------------------------------------------------------------------------------------------ the MOI getter
@pytest.mark.gpu
def test_moi_getter_returns_the_factor_of_a_psd_constraint():
    """sdp_from_moi (moi_proxsdp_unit.jl:184-223): X = ones(2, 2), rank one"""
    m = moi.Model()
    x = m.add_variables(3)
    ci = m.add_constraint(moi.VectorOfVariables(x), moi.PositiveSemidefiniteConeTriangle(2))
    ce = m.add_constraint(moi.ScalarAffineFunction([moi.ScalarAffineTerm(1.0, x[1])], 0.0), moi.EqualTo(1.0))
    m.set_objective_sense(moi.MIN_SENSE)
    m.set_objective_function(moi.ScalarAffineFunction([moi.ScalarAffineTerm(1.0, x[0]), moi.ScalarAffineTerm(1.0, x[2])], 0.0))
    m.optimize(factors=True)
    vals, vecs, info = m.constraint_primal_factor(ci)
    Xk = P.unpack_psd(m.constraint_primal(ci), 2)
    assert info["source"] == B.FACTOR_EIG and vecs.shape[0] == 2
    assert abs(info["resid"] - fro_resid(Xk, vals, vecs)) <= 64 * U * np.linalg.norm(Xk)
    assert np.allclose((vecs * vals) @ vecs.T, np.ones((2, 2)), atol=1e-3)
    with pytest.raises(TypeError):
        m.constraint_primal_factor(ce)
