"""The rounding of a kept model's factors on the GPU (proxsdp_hip_model_round; csrc/rounding.hip.hpp; binding.Model.round,
Optimizer.round): the device equals the NumPy restatement of rounding_cases.py EXACTLY -- signs, best_trial, value,
value_rounded, the values of every trial, sweeps, flips, and the adjacency against the one built from the caller's c -- on
both routes (host arrays, CUDA tensors), at every launch shape and with the word columns in LDS and in global memory; the
objective follows update(c=...); the handle is not touched; the device's refusals leave it usable; and a cutting-plane round
with a rounding before and after it runs end to end on a kept model.  Every comparison is an equality: no tolerance.

Sides.  A word holds 64 trials and a wave walks a node's row in pieces of 64: 2, 3, 4 and 16 are one ragged piece, 63 / 64 /
65 the edge, 130 three pieces; the sign kernel's tile of 16 nodes is ragged at all of them but 16 and 64.  One model holds a
Max-Cut cone of each side, its variables shuffled: no cone is the first variables, none is contiguous in the caller's order,
so every comparison also checks that the objective is read through the cone's variable list."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

import rounding_cases as R
from test_triangle_cuts import _assert_equal, _host, _opts

pytestmark = pytest.mark.gpu

SIDES = (2, 3, 4, 16, 63, 64, 65, 130)
E_INVALID = -1
OPTIMAL = 1
SMALLEST = dict(grid_adjacency=1, grid_directions=1, grid_signs=1, grid_search=1)


@functools.lru_cache(maxsize=None)
def _shapes_problem():
    """one Max-Cut block per side of SIDES, the variables of the whole model shuffled (test_triangle_cuts._shapes_problem)"""
    pr = P.block_diag_problems([P.maxcut(s, seed=s, avg_degree=4.0) for s in SIDES])
    perm = np.random.default_rng(13).permutation(pr.n)             # old variable v is new variable perm[v]
    inv = np.argsort(perm)
    return P.Problem(n=pr.n, A=sp.csc_matrix(pr.A)[:, inv], b=pr.b, G=sp.csc_matrix(pr.G)[:, inv], h=pr.h, c=pr.c[inv],
                     psd=[perm[v].astype(np.int64) for v in pr.psd], max_sense=pr.max_sense)


@pytest.fixture(scope="module")
def shapes():
    pr = _shapes_problem()
    with B.Model(pr, _opts(max_iter=12)) as mdl:
        yield pr, mdl


def _ranks(side):
    """r in {1, 17, s}, the last at side 4; the sides below 17 take 2 for 17"""
    return [1, 17 if side >= 17 else min(side, 2)] + ([4] if side == 4 else [])


@functools.lru_cache(maxsize=None)
def _adjacency(side, c_key=None):
    pr = _shapes_problem()
    return R.adjacency(pr.c[pr.psd[SIDES.index(side)]], side)


@functools.lru_cache(maxsize=None)
def _want(side, r, trials, seed, max_sweeps):
    """the restatement, once per case, shared by the routes and the knobs"""
    vals, V = R.factors(side, r, seed=side + r)
    return R.restate(vals, V, _adjacency(side), trials, seed, max_sweeps)


def _route(route, vals, V):
    if route == "device":
        return torch.as_tensor(vals, device="cuda:0"), torch.as_tensor(V, device="cuda:0")
    return vals, V


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("side", SIDES)
def test_device_equals_the_restatement(shapes, side, route):
    pr, mdl = shapes
    cone = SIDES.index(side)
    for a, r in enumerate(_ranks(side)):
        vals, V = R.factors(side, r, seed=side + r)
        for trials in (64, 192):
            ms = (50, 1, 0)[(a + trials // 64) % 3]
            got = mdl.round(_route(route, vals, V), cone=cone, trials=trials, seed=side, max_sweeps=ms, adjacency=True)
            R.assert_rounding_equal(got, _want(side, r, trials, side, ms), (side, route, r, trials, ms))
            for x, y in zip(got.adjacency, _adjacency(side)):
                assert x.dtype == y.dtype and np.array_equal(x, y), (side, route, "adjacency")
            assert got.bytes_allocated >= 8 * r * trials + 2 * 8 * side * (trials // 64) and got.search_seconds >= 0.0


@pytest.mark.parametrize("side", [16, 65, 130])
def test_the_result_does_not_depend_on_a_knob(shapes, side):
    """every launch at one workgroup, the word columns in global memory (lds_side=0: forced at side 130, where the default
    keeps them in LDS), and an LDS limit exactly at and just below the side"""
    pr, mdl = shapes
    cone = SIDES.index(side)
    r = 17 if side >= 17 else 2
    vals, V = R.factors(side, r, seed=side + r)
    for trials in (64, 192):
        want = _want(side, r, trials, side, 50)
        for knobs in (None, SMALLEST, dict(lds_side=0), dict(SMALLEST, lds_side=0), dict(lds_side=side), dict(lds_side=side - 1),
                      dict(grid_search=2, grid_signs=3, grid_adjacency=5, grid_directions=7)):
            for route in ("host", "device"):
                got = mdl.round(_route(route, vals, V), cone=cone, trials=trials, seed=side, max_sweeps=50, knobs=knobs)
                R.assert_rounding_equal(got, want, (side, trials, knobs, route))
                assert got.adjacency is None
    assert want["flips"] > 0 and want["sweeps"] >= 2               # (the search did something to be independent of)
    with pytest.raises(ValueError):
        mdl.round((vals, V), cone=cone, knobs=dict(grid_nothing=1))


@pytest.mark.parametrize("route", ["host", "device"])
def test_rounding_follows_an_update_of_c_with_real_weights(route):
    pr = _shapes_problem()
    rng = np.random.default_rng(5)
    c_new = np.where(pr.c != 0.0, rng.standard_normal(pr.n), 0.0)  # real weights on the model's own pattern
    c_new[pr.psd[SIDES.index(65)][::7]] = rng.standard_normal(len(pr.psd[SIDES.index(65)][::7]))      # and beyond it
    with B.Model(pr, _opts(max_iter=12)) as mdl:
        mdl.update(c=torch.as_tensor(c_new, device="cuda:0") if route == "device" else c_new)
        for side in (4, 65, 130):
            cone = SIDES.index(side)
            adj = R.adjacency(c_new[pr.psd[cone]], side)
            assert not np.array_equal(adj[2], _adjacency(side)[2])
            r = min(side, 17)
            vals, V = R.factors(side, r, seed=side + r)
            got = mdl.round(_route(route, vals, V), cone=cone, trials=192, seed=2, max_sweeps=50, adjacency=True)
            R.assert_rounding_equal(got, R.restate(vals, V, adj, 192, 2, 50), (side, route, "updated c"))
            for x, y in zip(got.adjacency, adj):
                assert np.array_equal(x, y), (side, route, "adjacency after the update")
        # back to the first objective: the rounding follows again
        mdl.update(c=pr.c)
        vals, V = R.factors(65, 17, seed=65 + 17)
        got = mdl.round(_route(route, vals, V), cone=SIDES.index(65), trials=64, seed=65, max_sweeps=50)
        R.assert_rounding_equal(got, _want(65, 17, 64, 65, 50), "first c again")


def test_the_handle_is_not_touched_and_refusals_leave_it_as_it_was(shapes):
    pr, mdl = shapes
    before = mdl.solve(trace_capacity=16, device_out=True, factors=True)
    info = mdl.info()
    cone = SIDES.index(65)
    vals, V = R.factors(65, 17, seed=65 + 17)
    want = _want(65, 17, 64, 65, 50)
    dv, dV = _route("device", vals, V)
    mdl.round((vals, V), cone=cone, trials=192, adjacency=True)
    mdl.round((dv, dV), cone=cone, trials=64, knobs=dict(lds_side=0))
    mdl.round(before, cone=SIDES.index(130), trials=64)             # the solve's own factors
    # ---- refusals that need the model or the device: each returns -1, and the next call works
    def refused(text, *a, **kw):
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.round(*a, **kw)
        assert e.value.code == E_INVALID and text in str(e.value), str(e.value)
        R.assert_rounding_equal(mdl.round((dv, dV), cone=cone, trials=64, seed=65), want, ("after", text))
    for bad in (np.nan, np.inf):
        y = V.copy()
        y[40, 9] = bad
        refused("V", (dv, torch.as_tensor(y, device="cuda:0")), cone=cone, trials=64)
        refused("V", (vals, y), cone=cone, trials=64)
    for bad in (0.0, -1.0, np.nan):
        y = vals.copy()
        y[16] = bad
        refused("values", (torch.as_tensor(y, device="cuda:0"), dV), cone=cone, trials=64)
        refused("values", (y, V), cone=cone, trials=64)
    refused("cone", (dv, dV), cone=-1, trials=64)
    refused("cone", (dv, dV), cone=len(SIDES), trials=64)
    refused("trials", (dv, dV), cone=cone, trials=96)
    v2, V2 = R.factors(2, 2, seed=0)
    with pytest.raises(ValueError):
        mdl.round((vals, dV), cone=cone)                            # host values with device vectors
    with pytest.raises(ValueError):
        mdl.round((v2, V2), cone=cone)                              # the wrong side
    # adj_cap one short of the adjacency: decided before any device call, nothing written
    nnz = int(_adjacency(65)[0][-1])
    Q, arr = B._rounding_struct(65, 17, 64, 65, 50, adj_cap=nnz, sentinel=7)     # (the arrays have room for all of it)
    Q.cone, Q.adj_cap = cone, nnz - 1
    keep = (np.ascontiguousarray(V.T).ravel(), vals)
    Q.V, Q.values = B._p(keep[0]), B._p(keep[1])
    assert nnz > 0 and B.lib().proxsdp_hip_model_round(mdl._handle(), Q) == E_INVALID
    assert all(np.all(a == 7) for a in arr.values())
    Q.adj_cap = nnz
    assert B.lib().proxsdp_hip_model_round(mdl._handle(), Q) == 0 and Q.adj_nnz == nnz
    R.assert_rounding_equal(B.Rounding(Q, arr), want, "adj_cap exactly the adjacency")
    after = mdl.solve(trace_capacity=16, device_out=True, factors=True)
    _assert_equal(after, before, "solve after the roundings")
    info2 = mdl.info()
    assert info2["device_bytes"] == info["device_bytes"] and info2["updates"] == info["updates"]


def _check_against_the_solve(pr, res, got, trials, seed, what):
    """value = c'x at the returned signs, recomputed (exact: dyadic weights), and the whole call = the restatement fed the
    solve's own factors"""
    vals, V = res.psd_factors[0][:2]
    assert got.value == R.cone_value(pr.c, got.signs), what
    R.assert_rounding_equal(got, R.restate(vals, V, R.adjacency(pr.c, 60), trials, seed, 50), what)
    assert got.value <= got.value_rounded and np.all(got.values_final <= got.values_rounded)


def test_rounding_before_and_after_a_cutting_plane_round_end_to_end():
    pr = P.maxcut(60, seed=0, avg_degree=4.0)
    with B.Model(pr, _opts()) as mdl:
        r0 = mdl.solve(device_out=True, factors=True)
        assert r0.status == OPTIMAL
        g0 = mdl.round(r0, trials=192, seed=1)
        _check_against_the_solve(pr, r0, g0, 192, 1, "first solution")
        cuts = mdl.separate_triangles(r0, count=20, min_violation=0.05)
        ch = mdl.change_rows(add=cuts.add)
        r1 = mdl.solve(start=ch.carry(r0), device_out=True, factors=True)
        assert r1.status == OPTIMAL
        g1 = mdl.round(r1, trials=192, seed=1)
        _check_against_the_solve(pr, r1, g1, 192, 1, "second solution")
        # a cut is a feasible point of the relaxation: the bound (minimisation form) lies below it, up to the solve's accuracy
        assert g1.value >= r1.objval - 1e-2 * abs(r1.objval)


def test_the_optimizer_rounds_on_its_kept_model():
    pr = P.maxcut(60, seed=0, avg_degree=4.0)
    opt = Optimizer()
    with pytest.raises(ValueError):
        opt.round()
    r0 = opt.optimize(pr, keep_model=True, factors=True)
    g0 = opt.round(trials=192, seed=1)
    _check_against_the_solve(pr, r0, g0, 192, 1, "optimizer, first solution")
    assert g0.objective == pr.user_objective(g0.value) == -g0.value and g0.objective <= r0.objval * (1 + 1e-2)
    cuts = opt.separate_triangles(count=20, min_violation=0.05)
    r1 = opt.reoptimize(add_rows=cuts.add, start=r0, factors=True)
    g1 = opt.round(trials=192, seed=1)
    _check_against_the_solve(pr, r1, g1, 192, 1, "optimizer, second solution")
    assert g1.objective == -g1.value
    opt.model.close()
