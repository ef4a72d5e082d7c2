"""The triangle separation and the slack-row entry on the GPU (proxsdp_hip_model_triangles, proxsdp_hip_model_inactive_rows;
csrc/triangle_cuts.hip.hpp; binding.Model.separate_triangles / inactive_rows): the device equals the NumPy brute force of
triangle_cases.py EXACTLY -- the rows, their order, the bits of the violations, add_col / add_val / add_h, n_rows, violated,
scanned -- on both routes (host array, CUDA tensor), at every launch shape of the sweep and with the refinement of the radix
select forced; the handle is not touched; and one cutting-plane round runs end to end on a kept model.

Sides.  The sweep's tile is 64 (triangle_cases.sweep_tile() reads it from the source and the test asserts it): 3 and 4 are one
ragged tile, 63 / 64 / 65 the tile edge, 130 three ragged tiles per dimension; 12 and 70 carry the all-equal matrices.  One
model holds a PSD cone of each side (and one of side 2 for the refusal), its variables shuffled: no cone is the first
variables, none is contiguous, so every comparison also checks add_col against the cone's variable list."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

import triangle_cases as T

pytestmark = pytest.mark.gpu

SIDES = (2, 3, 4, 12, 63, 64, 65, 70, 130)
GRAM_SEED = {3: 0, 4: 0, 63: 3, 64: 4, 65: 1, 130: 2}
E_INVALID = -1
OPTIMAL = 1
VECTORS = ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in")
SCALARS = ("status", "certificate_found", "primal_feasible_user_tol", "dual_feasible_user_tol", "result_count", "final_rank",
           "iter", "primal_residual", "dual_residual", "objval", "dual_objval", "gap", "dual_feasibility", "status_string")
INT_STATS = tuple(k for k, t in B.Stats._fields_ if t is B.i64) + ("reserved_s",)
TRACE_ELAPSED = 12


def _opts(**kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def _host(v):
    return v.cpu().numpy() if hasattr(v, "is_cuda") else np.asarray(v)


def _assert_equal(got, want, what):
    """test_model_rows.py's "equal", restated: everything but the clocks"""
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
        assert a.shape == b.shape and np.array_equal(a, b), (what, k)


@functools.lru_cache(maxsize=None)
def _shapes_problem():
    """one Max-Cut block per side of SIDES, the variables of the whole model shuffled"""
    pr = P.block_diag_problems([P.maxcut(s, seed=0, avg_degree=2.0) for s in SIDES])
    perm = np.random.default_rng(11).permutation(pr.n)             # old variable v is new variable perm[v]
    inv = np.argsort(perm)
    return P.Problem(n=pr.n, A=sp.csc_matrix(pr.A)[:, inv], b=pr.b, G=sp.csc_matrix(pr.G)[:, inv], h=pr.h, c=pr.c[inv],
                     psd=[perm[v].astype(np.int64) for v in pr.psd], max_sense=pr.max_sense)


@pytest.fixture(scope="module")
def shapes():
    pr = _shapes_problem()
    with B.Model(pr, _opts(max_iter=12)) as mdl:
        yield pr, mdl


def _primal(pr, side, X):
    """a primal vector of the shapes model with X in the cone of that side (the other cones: zeros)"""
    x = np.zeros(pr.n)
    x[pr.psd[SIDES.index(side)]] = T.pack(X)
    return x


@functools.lru_cache(maxsize=None)
def _gram(side):
    return T.gram(side, 3, GRAM_SEED[side])


@functools.lru_cache(maxsize=None)
def _want(side, count):
    """the brute force, once per (side, count), shared by the two routes"""
    return T.brute_force(_gram(side), count, cone_idx=_shapes_problem().psd[SIDES.index(side)])


def test_the_tile_is_the_one_the_sides_were_chosen_for():
    assert T.sweep_tile() == 64


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("side", [3, 4, 63, 64, 65, 130])
def test_device_equals_the_brute_force(shapes, side, route):
    pr, mdl = shapes
    cone = SIDES.index(side)
    x = _primal(pr, side, _gram(side))
    if route == "device":
        x = torch.as_tensor(x, device="cuda:0")
    for count in (1, 100, 1000):
        cuts = mdl.separate_triangles(x, cone=cone, count=count)
        T.assert_cuts_equal(cuts, _want(side, count), (side, route, count), raw_base=0)
        assert cuts.passes >= 1 and cuts.bytes_allocated >= 8 * side * side


def test_rhs_threshold_and_index_base_follow_the_brute_force(shapes):
    pr, mdl = shapes
    X, idx = _gram(65), pr.psd[SIDES.index(65)]
    x = torch.as_tensor(_primal(pr, 65, X), device="cuda:0")
    for kw in (dict(rhs=0.9), dict(min_violation=0.3), dict(rhs=1.2, min_violation=0.0)):
        cuts = mdl.separate_triangles(x, cone=SIDES.index(65), count=200, **kw)
        T.assert_cuts_equal(cuts, T.brute_force(X, 200, cone_idx=idx, **kw), kw)
    with B.Model(pr, _opts(max_iter=12), index_base=1) as m1:
        cuts = m1.separate_triangles(x, cone=SIDES.index(65), count=50)
        T.assert_cuts_equal(cuts, T.brute_force(X, 50, cone_idx=idx + 1), "index base 1", raw_base=1)


def test_forced_refinement_gives_the_same_rows_in_more_passes(shapes):
    pr, mdl = shapes
    cone = SIDES.index(65)
    x = torch.as_tensor(_primal(pr, 65, _gram(65)), device="cuda:0")
    plain = mdl.separate_triangles(x, cone=cone, count=50)
    forced = mdl.separate_triangles(x, cone=cone, count=50, cand_cap=64)
    want = T.brute_force(_gram(65), 50, cone_idx=pr.psd[cone])
    T.assert_cuts_equal(plain, want, "default cand_cap")
    T.assert_cuts_equal(forced, want, "cand_cap 64")
    assert forced.passes > plain.passes >= 2, (forced.passes, plain.passes)
    assert forced.bytes_allocated < plain.bytes_allocated


@pytest.mark.parametrize("side,count,cap", [(12, 5, 8), (70, 100, 128)])
def test_equal_violations_are_decided_by_the_index_digits(shapes, side, count, cap):
    pr, mdl = shapes
    cone = SIDES.index(side)
    X = T.ties(side)
    want = T.brute_force(X, count, cone_idx=pr.psd[cone])
    assert want["violated"] == side * (side - 1) * (side - 2) // 6 and np.all(want["violation"] == 0.5)
    for x in (_primal(pr, side, X), torch.as_tensor(_primal(pr, side, X), device="cuda:0")):
        cuts = mdl.separate_triangles(x, cone=cone, count=count, cand_cap=cap)
        T.assert_cuts_equal(cuts, want, ("ties", side))
        assert cuts.passes > 5                                     # the digits of v decide nothing: the index digits are walked
    # with room for every violated row the first histogram is enough
    cuts = mdl.separate_triangles(_primal(pr, side, X), cone=cone, count=count)
    T.assert_cuts_equal(cuts, want, ("ties", side, "default"))
    assert cuts.passes == 2


def test_a_cut_matrix_violates_nothing(shapes):
    pr, mdl = shapes
    x = torch.as_tensor(_primal(pr, 65, T.feasible(65)), device="cuda:0")
    cuts = mdl.separate_triangles(x, cone=SIDES.index(65), count=100)
    assert len(cuts) == 0 and cuts.violated == 0 and cuts.scanned == 4 * 43680 and cuts.passes == 1
    (ptr, cols, vals), h = cuts.add
    assert ptr.tolist() == [0] and len(cols) == 0 and len(vals) == 0 and len(h) == 0


def test_the_handle_is_not_touched_and_refusals_leave_it_as_it_was(shapes):
    pr, mdl = shapes
    before = mdl.solve(trace_capacity=16, device_out=True)
    info = mdl.info()
    cone = SIDES.index(65)
    x = _primal(pr, 65, _gram(65))
    xd = torch.as_tensor(x, device="cuda:0")
    mdl.separate_triangles(x, cone=cone, count=100)
    mdl.separate_triangles(xd, cone=cone, count=100, cand_cap=128)
    mdl.separate_triangles(before, cone=SIDES.index(130), count=10, min_violation=0.0)
    for what, kw, text in (("side 2", dict(cone=SIDES.index(2)), "side < 3"), ("cone -1", dict(cone=-1), "cone"),
                           ("cone past the end", dict(cone=len(SIDES)), "cone")):
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.separate_triangles(xd, **kw)
        assert e.value.code == E_INVALID and text in str(e.value), (what, str(e.value))
    for bad in (np.nan, np.inf):
        for route in (lambda v: v, lambda v: torch.as_tensor(v, device="cuda:0")):
            y = x.copy()
            y[pr.psd[cone][1234]] = bad
            with pytest.raises(B.ProxSDPHipError) as e:
                mdl.separate_triangles(route(y), cone=cone)
            assert e.value.code == E_INVALID and "non-finite" in str(e.value) and f"cone {cone}" in str(e.value)
            # a non-finite entry OUTSIDE the cone is none of this call's business
            y = x.copy()
            y[pr.psd[SIDES.index(130)][7]] = bad
            T.assert_cuts_equal(mdl.separate_triangles(route(y), cone=cone, count=100), _want(65, 100), "outside the cone")
    with pytest.raises(ValueError):
        mdl.separate_triangles(x[:-1], cone=cone)
    after = mdl.solve(trace_capacity=16, device_out=True)
    _assert_equal(after, before, "solve after the separations")
    info2 = mdl.info()
    assert info2["device_bytes"] == info["device_bytes"] and info2["updates"] == info["updates"]


def test_one_cutting_plane_round_end_to_end():
    """P.maxcut(60, seed=0, avg_degree=6.0), default options.  The CPU oracle on the same two problems: the first solution
    (705 iterations, OPTIMAL) has 14 793 rows above 0.05 (largest 0.4986); with the 20 most violated added the second solve
    ends OPTIMAL (1015 iterations from a cold start) and leaves at most 5.4e-4 on the added rows."""
    pr = P.maxcut(60, seed=0, avg_degree=6.0)
    with B.Model(pr, _opts()) as mdl:
        r0 = mdl.solve(device_out=True, factors=True)
        assert r0.status == OPTIMAL
        cuts = mdl.separate_triangles(r0, count=20, min_violation=0.05)
        X0 = P.unpack_psd(_host(r0.primal), 60)
        T.assert_cuts_equal(cuts, T.brute_force(X0, 20, min_violation=0.05), "first solution", raw_base=0)
        assert len(cuts) == 20
        ch = mdl.change_rows(add=cuts.add)
        assert ch.m == 20
        r1 = mdl.solve(start=ch.carry(r0), device_out=True)
        assert r1.status == OPTIMAL
        X1 = P.unpack_psd(_host(r1.primal), 60)
        added = {(tuple(t), int(p)) for t, p in zip(cuts.triples.tolist(), cuts.patterns.tolist())}
        for (i, j, k), p in added:
            s = T.SIGNS[p]
            assert ((s[0] * X1[i, j] + s[1] * X1[i, k]) + s[2] * X1[j, k]) - 1.0 < 0.05, (i, j, k, p)
        again = mdl.separate_triangles(r1, count=1000, min_violation=0.05)
        T.assert_cuts_equal(again, T.brute_force(X1, 1000, min_violation=0.05), "second solution")
        assert not added & {(tuple(t), int(p)) for t, p in zip(again.triples.tolist(), again.patterns.tolist())}
        rows = mdl.inactive_rows(r1)
        d, s = _host(r1.dual_in), _host(r1.slack_in)
        assert rows.dtype == np.int64 and np.all(np.diff(rows) > 0) and np.all((rows >= 0) & (rows < 20))
        assert np.array_equal(rows, np.nonzero((np.abs(d) <= 0.0) & (s < -1e-6))[0])
        assert np.array_equal(mdl.inactive_rows((d, s)), rows)


def test_the_optimizer_runs_the_round_on_its_kept_model():
    pr = P.maxcut(60, seed=0, avg_degree=6.0)
    opt = Optimizer()
    r0 = opt.optimize(pr, keep_model=True)
    cuts = opt.separate_triangles(count=20, min_violation=0.05)
    X0 = P.unpack_psd(_host(r0.primal), 60)
    T.assert_cuts_equal(cuts, T.brute_force(X0, 20, min_violation=0.05), "optimizer")
    r1 = opt.reoptimize(add_rows=cuts.add, start=r0)
    assert r1.status == OPTIMAL and opt.problem.G.shape[0] == 20
    rows = opt.inactive_rows()
    assert np.array_equal(rows, np.nonzero((np.abs(_host(r1.dual_in)) <= 0.0) & (_host(r1.slack_in) < -1e-6))[0])
    r2 = opt.reoptimize(drop_rows=rows, start=r1) if len(rows) else r1
    assert r2.status == OPTIMAL and opt.problem.G.shape[0] == 20 - len(rows)
    opt.model.close()


# ----------------------------------------------------------------- the slack rows alone
DUAL_TOL, SLACK_TOL = 1e-8, 1e-3


def _crafted(m, seed):
    """duals and slacks drawn from the values at, next to and far from both thresholds, and NaN"""
    rng = np.random.default_rng(seed)
    dv = np.array([0.0, -0.0, DUAL_TOL, -DUAL_TOL, np.nextafter(DUAL_TOL, 1.0), -np.nextafter(DUAL_TOL, 1.0), 0.5, np.nan])
    sv = np.array([-SLACK_TOL, np.nextafter(-SLACK_TOL, -1.0), np.nextafter(-SLACK_TOL, 0.0), -1.0, 0.0, 2.0, np.nan])
    d, s = dv[rng.integers(0, len(dv), m)], sv[rng.integers(0, len(sv), m)]
    k = min(m, len(dv))
    d[:k], s[:k] = dv[:k], sv[1]                                  # every dual value against a slack that passes
    return d, s


def _inactive(d, s, dual_tol, slack_tol):
    with np.errstate(invalid="ignore"):
        return np.nonzero((np.abs(d) <= dual_tol) & (s < -slack_tol))[0].astype(np.int64)


@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 1000, 1023, 1024, 1025, 2500])
def test_inactive_rows_equal_numpy_on_both_routes(m):
    """255 / 256 / 257 and 1000 are the issue's; the kernel walks the rows in pieces of 1024 (INACT_TPB), so 1023 / 1024 / 1025
    are its edge and 2500 is three pieces, the last one ragged"""
    base = P.maxcut_readme()
    rng = np.random.default_rng(m)
    G = sp.csc_matrix((np.ones(m), (np.arange(m), rng.integers(0, base.n, m))), shape=(m, base.n))
    pr = P.Problem(n=base.n, A=base.A, b=base.b, G=G, h=np.full(m, 10.0), c=base.c, psd=base.psd, max_sense=True)
    d, s = _crafted(m, m)
    with B.Model(pr, _opts()) as mdl:
        for dt, st in ((DUAL_TOL, SLACK_TOL), (0.0, 0.0), (0.5, 1.0)):
            want = _inactive(d, s, dt, st)
            got_h = mdl.inactive_rows((d, s), dual_tol=dt, slack_tol=st)
            got_d = mdl.inactive_rows((torch.as_tensor(d, device="cuda:0"), torch.as_tensor(s, device="cuda:0")), dual_tol=dt, slack_tol=st)
            assert got_h.dtype == np.int64 and np.array_equal(got_h, want), (m, dt, st, "host")
            assert got_d.dtype == np.int64 and np.array_equal(got_d, want), (m, dt, st, "device")
        if m >= 8:
            want = _inactive(d, s, DUAL_TOL, SLACK_TOL)
            # at the thresholds: |dual| == dual_tol is inactive, slack == -slack_tol is not, NaN never is
            assert {0, 1, 2, 3} <= set(want.tolist()) and not {4, 5, 6, 7} & set(want.tolist())
            assert not set(np.nonzero(s == -SLACK_TOL)[0].tolist()) & set(want.tolist())
            assert not set(np.nonzero(np.isnan(d) | np.isnan(s))[0].tolist()) & set(want.tolist())
        with pytest.raises(ValueError):
            mdl.inactive_rows((d, torch.as_tensor(s, device="cuda:0")))
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.inactive_rows((d, s), dual_tol=-1.0)
        assert e.value.code == E_INVALID
