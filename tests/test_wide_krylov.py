"""Wide Lanczos (options.lanczos_wide_krylov = 1): Krylov dimensions 256..511 run on the device instead of the dense
stand-in.  Against the CPU oracle (KrylovKit's thick restart restated in NumPy) and LAPACK."""
import numpy as np
import pytest

import oracle
from oracle import Options, eig as oeig
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

from helpers import oracle_project, planted_packed, smat, svec

pytestmark = pytest.mark.gpu

COLS = [1, 2, 3, 4, 7, 11]
NOT_TIME = [c for c in range(14) if c != 12]       # trace column 12 is wall-clock time


def _trace_cols(ref_trace):
    return np.array([[t["prim_obj"], t["dual_obj"], t["gap"], t["feas"], t["primal_step"], t["trials"]]
                     for t in ref_trace])


def _counts_match(got, exp):
    """per-iteration Lanczos mat-vec counts: the wide kernels measure both Gram-Schmidt passes (the oracle subtracts the known
    recurrence terms in its first pass), so a convergence test that sits at krylovkit_tol can flip by one step pair in an
    isolated iteration; everything else is equal"""
    got, exp = np.asarray(got, float), np.asarray(exp, float)
    diff = np.flatnonzero(got != exp)
    return len(diff) <= 2 and bool(np.all(np.abs(got[diff] - exp[diff]) <= 0.01 * exp[diff]))


def _wide(**kw):
    o = B.default_options()
    B.set_option(o, "lanczos_wide_krylov", 1)
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def _check_eigsolve(n, nev, K, top, bulk, seed):
    x = planted_packed(n, seed, top, bulk=bulk)
    X = smat(x, n)
    scale = max(abs(top[0]), abs(bulk[0]), abs(bulk[1]))
    vals, vecs, info = B.eigsolve(x, n, nev, options=_wide(eigsolver_min_lanczos=K if K > 2 * nev + 1 else 25),
                                  cap=K + 1)
    ovals, ovecs, oconv, onumiter, onumops = oeig.krylovkit_eigsolve(lambda v: X @ v, oeig.start_vector(n), nev, K,
                                                                     100, 1e-12)
    assert info["numiter"] == onumiter and info["nmatvec"] == onumops, (n, nev, K, info, onumiter, onumops)
    k = min(len(vals), len(ovals), nev)
    assert k == nev
    lap = np.sort(np.linalg.eigvalsh(X))[::-1]
    assert np.abs(vals[:k] - lap[:k]).max() <= 1e-11 * scale
    assert np.abs(vals[:k] - ovals[:k]).max() <= 1e-11 * scale
    V = vecs[:, :k]
    assert np.abs(X @ V - V * vals[:k]).max() <= 1e-9 * scale
    assert np.abs(V.T @ V - np.eye(k)).max() <= 1e-10
    return info


@pytest.mark.parametrize("n,nev,K", [(700, 130, 261), (1000, 160, 321), (1500, 200, 401), (2000, 255, 511)])
def test_wide_eigsolve_matches_lapack_and_oracle_counts(n, nev, K):
    top = list(np.linspace(80.0, 5.0, nev + 20))
    _check_eigsolve(n, nev, K, top, (-3.0, 0.5), 3 + n)


def test_wide_eigsolve_clustered_spectrum_restarts():
    """a clustered top of the spectrum: more than one cycle, i.e. the wide restart rotation runs"""
    nev, n = 130, 800
    top = list(np.linspace(60.0, 40.0, nev + 40))
    info = _check_eigsolve(n, nev, 261, top, (-1.0, 39.9), 17)
    assert info["numiter"] > 1


def test_wide_eigsolve_min_lanczos_300_and_arpack_rule():
    top = [40.0, 30.0, 20.0, 10.0, 9.0, 8.0]
    _check_eigsolve(600, 4, 300, top, (-5.0, 1.0), 5)
    # ARPACK's acceptance rule (eigsolver = 1) on the same engine at K = 301
    n, nev = 700, 150
    x = planted_packed(n, 9, list(np.linspace(60.0, 2.0, nev + 10)), bulk=(-3.0, 0.5))
    vals, vecs, info = B.eigsolve(x, n, nev, options=_wide(eigsolver=1), cap=nev + 2)
    assert info["converged"] >= nev
    lap = np.sort(np.linalg.eigvalsh(smat(x, n)))[::-1][:nev]
    assert np.abs(np.sort(vals[:nev])[::-1] - lap).max() <= 1e-9 * 60.0


def test_wide_maxcut_n400_rank150_against_oracle():
    """the dense stand-in's case (krylovdim 301) with the option on: Lanczos on the device, the oracle's counts"""
    pr = P.maxcut(400, seed=1)
    kw = dict(max_target_rank_krylov_eigs=200, initial_target_rank=150, max_iter=25)
    sol = Optimizer(lanczos_wide_krylov=1, **kw).optimize(pr, trace_capacity=25)
    o = Options()
    o.max_target_rank_krylov_eigs, o.initial_target_rank, o.max_iter = 200, 150, 25
    omv = []
    ref = oracle.solve(pr, o, trace=True, proj_callback=lambda it, xi, xo, p_, arc: omv.append(int(arc[0].matvecs)))
    assert sol.status == ref.status and sol.iter == ref.iter == 25
    per_it = np.diff(np.array([0] + omv))
    assert _counts_match(sol.trace[:, 13], per_it), (sol.trace[:, 13], per_it)
    assert np.allclose(sol.trace[:, COLS], _trace_cols(ref.trace), rtol=1e-8, atol=1e-10)
    assert sol.stats["dense_truncated_projections"] == 0 and sol.stats["wide_krylov_projections"] == 25
    assert sol.stats["lanczos_matvecs"] == int(sol.trace[:, 13].sum())
    assert sol.final_rank == ref.final_rank
    assert "dense eigensolver served" not in sol.status_string


def test_wide_maxcut_n1000_rank130_longer_solve():
    """a solve whose rank schedule runs through min_eig (the minimum over every returned value, prox_operators.jl:95)"""
    pr = P.maxcut(1000, seed=2)
    iters = 80
    kw = dict(max_target_rank_krylov_eigs=140, initial_target_rank=130, max_iter=iters)
    sol = Optimizer(lanczos_wide_krylov=1, **kw).optimize(pr, trace_capacity=iters)
    o = Options()
    o.max_target_rank_krylov_eigs, o.initial_target_rank, o.max_iter = 140, 130, iters
    omv = []
    ref = oracle.solve(pr, o, trace=True, proj_callback=lambda it, xi, xo, p_, arc: omv.append(int(arc[0].matvecs)))
    assert sol.status == ref.status and sol.iter == ref.iter
    per_it = np.diff(np.array([0] + omv))
    assert _counts_match(sol.trace[:, 13], per_it), (sol.trace[:, 13], per_it)
    G = _trace_cols(ref.trace)
    assert np.allclose(sol.trace[:, COLS], G, rtol=1e-8, atol=1e-10 * np.abs(G).max())
    assert sol.final_rank == ref.final_rank
    # the rank schedule (target rank after each iteration's min_eig / current_rank test) is the oracle's, iteration by iteration
    assert np.array_equal(sol.trace[:, 10], np.array([t["target_rank"][0] for t in ref.trace], float))
    assert sol.stats["wide_krylov_projections"] == iters and sol.stats["dense_truncated_projections"] == 0


def test_wide_limits_and_guards():
    pr = P.maxcut(400, seed=1)
    # Krylov dimension beyond 511: still the dense stand-in, counted
    sol = Optimizer(lanczos_wide_krylov=1, max_target_rank_krylov_eigs=300, initial_target_rank=300,
                    max_iter=5).optimize(pr, trace_capacity=5)
    assert sol.stats["dense_truncated_projections"] == 5 and sol.stats["wide_krylov_projections"] == 0
    # Krylov dimension <= 255: the option changes nothing
    a = Optimizer(max_iter=40).optimize(pr, trace_capacity=40)
    b = Optimizer(max_iter=40, lanczos_wide_krylov=1).optimize(pr, trace_capacity=40)
    assert np.array_equal(a.trace[:, NOT_TIME], b.trace[:, NOT_TIME])
    # every counter of the stats (the float fields are times, profiled milliseconds and byte estimates)
    counters = [f for f, t in B.Stats._fields_ if t is B.i64]
    assert {f: a.stats[f] for f in counters} == {f: b.stats[f] for f in counters}
    assert b.stats["wide_krylov_projections"] == 0 and b.stats["lanczos_matvecs"] > 0
    # values other than 0 / 1 are refused
    with pytest.raises(Exception):
        Optimizer(lanczos_wide_krylov=2, max_iter=2).optimize(pr)


def test_wide_two_block_model_with_and_without_block_workers():
    """one wide block (side 400, target rank 140: Krylov dimension 281) next to a narrow one (side 120: its target rank is
    capped at the side, Krylov dimension 241 on the step kernels), with and without the block worker pool"""
    pr = P.block_diag_problems([P.maxcut(400, seed=1), P.maxcut(120, seed=4)])
    kw = dict(max_target_rank_krylov_eigs=200, initial_target_rank=140, max_iter=15)
    o = Options()
    o.max_target_rank_krylov_eigs, o.initial_target_rank, o.max_iter = 200, 140, 15
    ref = oracle.solve(pr, o, trace=True)
    G = _trace_cols(ref.trace)
    sols = [Optimizer(lanczos_wide_krylov=1, block_threads=bt, **kw).optimize(pr, trace_capacity=15) for bt in (0, -1)]
    for sol in sols:
        assert sol.status == ref.status and sol.iter == ref.iter
        assert np.allclose(sol.trace[:, COLS], G, rtol=1e-8, atol=1e-10 * np.abs(G).max())
        # per iteration: one projection of the wide block on the wide kernels, one of the narrow block on the step kernels
        assert sol.stats["wide_krylov_projections"] == 15 and sol.stats["dense_truncated_projections"] == 0
        assert sol.stats["lanczos_calls"] == 30
    assert np.array_equal(sols[0].trace[:, NOT_TIME], sols[1].trace[:, NOT_TIME])


# ----------------------------------------------------------------- edge cases of the wide engine (as test_lanczos_edge_cases
# for the step kernels)
@pytest.mark.parametrize("n", [576, 1024])
def test_wide_eigsolve_sides_multiple_of_64(n):
    """no padding rows: the last row group is full"""
    _check_eigsolve(n, 130, 261, list(np.linspace(80.0, 5.0, 150)), (-3.0, 0.5), 40 + n)


@pytest.mark.parametrize("n,nev", [(260, 130), (300, 150)])
def test_wide_eigsolve_krylov_dimension_beyond_n(n, nev):
    """Krylov dimension 2 nev + 1 > n: the Krylov space runs out inside the first cycle"""
    _check_eigsolve(n, nev, 2 * nev + 1, list(np.linspace(50.0, 10.0, nev + 10)), (-2.0, 1.0), 60 + n)


def test_wide_eigsolve_zero_matrix():
    """invariant subspace at K = 1, howmany reduced -- the step kernels' case in test_lanczos_edge_cases"""
    vals, vecs, info = B.eigsolve(np.zeros(300 * 301 // 2), 300, 130, options=_wide())
    assert list(vals) == [0.0] and info["converged"] == 1 and info["nmatvec"] == 1


def test_wide_eigsolve_exact_low_rank_stops_mid_cycle():
    """a rank-5 PSD matrix: the Krylov space has dimension 6, so the engine stops at step 6 of a 261-step cycle; values,
    vectors and counts as the oracle's"""
    n, nev = 600, 130
    rng = np.random.default_rng(21)
    Z, _ = np.linalg.qr(rng.standard_normal((n, 5)))
    lam = np.array([9.0, 7.0, 4.0, 2.5, 1.0])
    X = (Z * lam) @ Z.T
    X = (X + X.T) / 2
    x = svec(X)
    vals, vecs, info = B.eigsolve(x, n, nev, options=_wide(), cap=262)
    ovals, ovecs, oconv, onumiter, onumops = oeig.krylovkit_eigsolve(lambda v: X @ v, oeig.start_vector(n), nev, 261,
                                                                     100, 1e-12)
    assert info["numiter"] == onumiter and info["nmatvec"] == onumops, (info, onumiter, onumops)
    assert onumops < 261
    assert len(vals) == len(ovals) and info["converged"] == oconv
    assert np.abs(vals - ovals).max() <= 1e-12 * 9.0
    assert np.abs(vals[:5] - lam).max() <= 1e-12 * 9.0
    assert np.abs(X @ vecs - vecs * vals).max() <= 1e-10 * 9.0
    assert np.abs(vecs.T @ vecs - np.eye(len(vals))).max() <= 1e-10


def test_wide_eigsolve_explicit_start_vector_and_determinism():
    n, nev = 700, 130
    x = planted_packed(n, 23, list(np.linspace(60.0, 5.0, nev + 10)), bulk=(-3.0, 0.5))
    r = np.random.default_rng(5).standard_normal(n)
    v1, z1, i1 = B.eigsolve(x, n, nev, options=_wide(), resid=r)
    v2, z2, i2 = B.eigsolve(x, n, nev, options=_wide(), resid=3.0 * r)   # normalised inside, as KrylovKit does
    assert np.allclose(v1[:nev], v2[:nev], rtol=0, atol=1e-12 * 60.0) and i1["nmatvec"] == i2["nmatvec"]
    X = smat(x, n)
    ovals, _, _, onumiter, onumops = oeig.krylovkit_eigsolve(lambda v: X @ v, r / np.linalg.norm(r), nev, 261, 100, 1e-12)
    assert i1["nmatvec"] == onumops and i1["numiter"] == onumiter
    assert np.abs(v1[:nev] - ovals[:nev]).max() <= 1e-11 * 60.0
    # fixed-order sums: two identical calls give the same bits
    v3, z3, i3 = B.eigsolve(x, n, nev, options=_wide(), resid=r)
    assert np.array_equal(v1, v3) and np.array_equal(z1, z3) and i1 == i3


def test_wide_psd_project_rank130_against_oracle():
    n, tr = 600, 130
    x = planted_packed(n, 29, list(np.linspace(70.0, 3.0, tr + 15)), bulk=(-4.0, 0.5))
    out, info = B.psd_project(x, n, tr, mode=0, options=_wide())
    o_out, o_rank, o_min, arc = oracle_project(x, n, tr, False)
    scale = np.abs(x).max()
    assert np.allclose(out, o_out, rtol=0, atol=2e-9 * scale), np.abs(out - o_out).max()
    assert info["rank"] == o_rank and info["fell_back"] == 0
    assert abs(info["min_eig"] - o_min) <= 1e-9 * scale
    assert info["nmatvec"] == arc.matvecs


@pytest.mark.parametrize("min_lanczos", [255, 256, 259])
def test_wide_engine_boundary_min_lanczos(min_lanczos):
    """Krylov dimension max(2 nev + 1, eigsolver_min_lanczos): 255 stays on the step kernels (their 4 waves x 64 basis
    columns), 256 is the first wide one, and 259 (the last that fits the step kernels' record stride) is wide too"""
    pr = P.maxcut(300, seed=3)
    iters = 15
    sol = Optimizer(lanczos_wide_krylov=1, eigsolver_min_lanczos=min_lanczos, max_iter=iters).optimize(
        pr, trace_capacity=iters)
    o = Options()
    o.max_iter, o.eigsolver_min_lanczos = iters, min_lanczos
    omv = []
    ref = oracle.solve(pr, o, trace=True, proj_callback=lambda it, xi, xo, p_, arc: omv.append(int(arc[0].matvecs)))
    assert sol.status == ref.status and sol.iter == ref.iter == iters
    per_it = np.diff(np.array([0] + omv))
    assert _counts_match(sol.trace[:, 13], per_it), (sol.trace[:, 13], per_it)
    G = _trace_cols(ref.trace)
    assert np.allclose(sol.trace[:, COLS], G, rtol=1e-8, atol=1e-10 * np.abs(G).max())
    assert sol.stats["wide_krylov_projections"] == (0 if min_lanczos == 255 else iters)
    assert sol.stats["dense_truncated_projections"] == 0
