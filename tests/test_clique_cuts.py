"""The pentagonal / heptagonal separation on the GPU (proxsdp_hip_model_cliques; csrc/clique_cuts.hip.hpp;
binding.Model.separate_cliques): the device equals the NumPy restatement of clique_cases.py EXACTLY -- the rows, their order,
the bits of the violations, from_base, add_col / add_val / add_h, n_rows, violated_bases, scanned -- on both routes (host
array, CUDA tensor), for every shape of a batch of bases and whatever the knobs are; the handle is not touched; and one round
past the triangles runs end to end on a kept model.

Sides.  The sweep's tile is 64 (clique_cases.sweep_tile() reads it from the source and the test asserts it): 5 and 7 are the
smallest sides of the two base sizes, 63 / 64 / 65 the tile edge, 130 three ragged tiles per dimension; 70 carries the
all-equal matrix and the planted pentagon.  A workgroup of the sweep owns 64 bases, one per lane: 1, 63, 64, 65 and 200 bases
are one lane, a ragged wave, a full wave, a wave plus one lane and several waves.  One model holds a PSD cone of each side
(and of sides 4 and 6 for the refusals), its variables shuffled: no cone is the first variables, none is contiguous, so every
comparison also checks add_col against the cone's variable list."""
import functools
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

import clique_cases as K
import triangle_cases as T
pytestmark = pytest.mark.gpu

SIDES = (4, 5, 6, 7, 63, 64, 65, 70, 130)
GRAM_SEED = {5: 0, 7: 0, 63: 3, 64: 4, 65: 1, 130: 2}               # (63 .. 130: the seeds of test_triangle_cuts.py)
N_BASE = (1, 63, 64, 65, 200)
PENTAGON_70 = (3, 20, 64, 65, 69)                                    # straddles the tile edge
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
    """test_triangle_cuts.py's "equal", restated: everything but the clocks"""
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


def _idx(side):
    return _shapes_problem().psd[SIDES.index(side)]


def _primal(side, X, device=False):
    """a primal vector of the shapes model with X in the cone of that side (the other cones: zeros)"""
    pr = _shapes_problem()
    x = np.zeros(pr.n)
    x[_idx(side)] = T.pack(X)
    return torch.as_tensor(x, device="cuda:0") if device else x


@functools.lru_cache(maxsize=None)
def _gram(side):
    return T.gram(side, 3, GRAM_SEED[side])


@functools.lru_cache(maxsize=None)
def _triangles(side):
    """the 200 triangle rows with the largest left sides, violated or not (all of them on sides 5 and 7)"""
    return T.brute_force(_gram(side), 200, min_violation=-10)


def _counts(side):
    return sorted({min(n, _triangles(side)["n_rows"]) for n in N_BASE})


@functools.lru_cache(maxsize=None)
def _want3(side, n_base):
    """the restatement, once per (side, n_base), shared by the two routes and the knobs"""
    return K.restatement(_gram(side), K.bases_from_triangles(_triangles(side), n_base), cone_idx=_idx(side))


@functools.lru_cache(maxsize=None)
def _want5(side):
    """heptagons from the pentagons of the most bases"""
    w = _want3(side, _counts(side)[-1])
    return K.restatement(_gram(side), (w["nodes"], w["signs"]), cone_idx=_idx(side))


def test_the_tile_and_the_wave_are_the_ones_the_shapes_were_chosen_for():
    assert K.sweep_tile() == 64 and K.sweep_wave() == 64


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("side", [5, 7, 63, 64, 65, 130])
def test_device_equals_the_restatement(shapes, side, route):
    pr, mdl = shapes
    cone = SIDES.index(side)
    x = _primal(side, _gram(side), device=route == "device")
    for n_base in _counts(side):
        cuts = mdl.separate_cliques(x, K.bases_from_triangles(_triangles(side), n_base), cone=cone)
        K.assert_cliques_equal(cuts, _want3(side, n_base), (side, route, n_base), raw_base=0)
        assert cuts.size == 5 and cuts.bytes_allocated >= 8 * side * side + 8 * side * 64 and cuts.sweep_seconds > 0.0
    if side >= 63:
        assert len(cuts) >= 190, len(cuts)                           # nearly every one of the 200 bases grows into a row of its own
    if side >= 7:
        hept = mdl.separate_cliques(x, cuts, cone=cone)              # a CliqueCuts of size 5 is a set of bases; rhs 3
        K.assert_cliques_equal(hept, _want5(side), (side, route, "q = 5"), raw_base=0)
        assert hept.size == 7 and np.all(hept.raw["add_h"] == 3.0) and (side < 63 or len(hept) >= 150)


@pytest.mark.parametrize("side", [65, 130])
def test_grid_and_batch_are_invisible(shapes, side):
    pr, mdl = shapes
    cone = SIDES.index(side)
    x = _primal(side, _gram(side), device=True)
    bases3 = K.bases_from_triangles(_triangles(side), 200)
    bases5 = (_want3(side, 200)["nodes"], _want3(side, 200)["signs"])
    for knobs in (None, dict(grid=1), dict(grid=7), dict(batch=64), dict(grid=2, batch=100), dict(grid=100000, batch=70000)):
        K.assert_cliques_equal(mdl.separate_cliques(x, bases3, cone=cone, knobs=knobs), _want3(side, 200), (side, knobs))
        K.assert_cliques_equal(mdl.separate_cliques(x, bases5, cone=cone, knobs=knobs), _want5(side), (side, knobs, "q = 5"))
    small = mdl.separate_cliques(x, bases3, cone=cone, knobs=dict(grid=1, batch=64))
    assert small.bytes_allocated < mdl.separate_cliques(x, bases3, cone=cone).bytes_allocated


def test_equal_values_are_decided_by_the_order_of_the_pairs_across_tiles(shapes):
    pr, mdl = shapes
    side, cone = 70, SIDES.index(70)
    X = T.ties(side)
    ones = lambda n, q: np.ones((n, q), dtype=np.int8)
    tri = (np.array([[0, 1, 2], [3, 4, 5], [0, 2, side - 1]], dtype=np.int64), ones(3, 3))
    pent = (np.arange(5, dtype=np.int64)[None, :], ones(1, 5))
    want3, want5 = K.restatement(X, tri, cone_idx=_idx(side)), K.restatement(X, pent, cone_idx=_idx(side))
    assert want3["nodes"].tolist() == [[0, 1, 2, 3, 4], [0, 1, 3, 4, 5], [0, 1, 2, 3, side - 1]] and np.all(want3["violation"] == 3.0)
    assert want5["nodes"].tolist() == [[0, 1, 2, 3, 4, 5, 6]] and want5["violation"].tolist() == [7.5]
    for x in (_primal(side, X), _primal(side, X, device=True)):
        for knobs in (None, dict(grid=1), dict(grid=3)):             # the winner is in the first tile; every other tile equals it
            K.assert_cliques_equal(mdl.separate_cliques(x, tri, cone=cone, knobs=knobs), want3, ("ties", knobs))
            K.assert_cliques_equal(mdl.separate_cliques(x, pent, cone=cone, knobs=knobs), want5, ("ties, q = 5", knobs))


def test_the_triangles_of_a_planted_pentagon_merge_into_one_row(shapes):
    pr, mdl = shapes
    side, cone = 70, SIDES.index(70)
    X = K.planted(side, PENTAGON_70)
    tri = np.array(list(itertools.combinations(PENTAGON_70, 3)), dtype=np.int64)
    bases = (tri, np.ones_like(tri, dtype=np.int8))
    want = K.restatement(X, bases, cone_idx=_idx(side))
    assert want["n_rows"] == 1 and want["violated_bases"] == 10 and want["nodes"].tolist() == [list(PENTAGON_70)]
    assert np.all(want["values"] > 0.5 - 1e-12)
    for x in (_primal(side, X), _primal(side, X, device=True)):
        for knobs in (None, dict(grid=2)):
            cuts = mdl.separate_cliques(x, bases, cone=cone, knobs=knobs)
            K.assert_cliques_equal(cuts, want, ("planted", knobs))
            assert cuts.from_base.tolist() == [int(np.flatnonzero(want["values"] == want["values"].max())[0])]
    # a cut matrix yields no row from any base
    cuts = mdl.separate_cliques(_primal(side, T.feasible(side), device=True), bases, cone=cone, min_violation=0.0)
    assert len(cuts) == 0 and cuts.violated_bases == 0 and cuts.scanned == 10 * 4 * (67 * 66 // 2)
    (ptr, cols, vals), h = cuts.add
    assert ptr.tolist() == [0] and len(cols) == 0 and len(vals) == 0 and len(h) == 0


def test_rhs_threshold_and_index_base_follow_the_restatement(shapes):
    pr, mdl = shapes
    X, idx, cone = _gram(65), _idx(65), SIDES.index(65)
    x = _primal(65, X, device=True)
    bases = K.bases_from_triangles(_triangles(65), 200)
    middle = float(np.median(_want3(65, 200)["violation"]))          # a threshold that turns about half of the bases away
    for kw in (dict(rhs=1.9), dict(min_violation=middle), dict(rhs=2.2, min_violation=0.0)):
        K.assert_cliques_equal(mdl.separate_cliques(x, bases, cone=cone, **kw), K.restatement(X, bases, cone_idx=idx, **kw), kw)
    assert 0 < K.restatement(X, bases, min_violation=middle)["n_rows"] < _want3(65, 200)["n_rows"]
    with B.Model(pr, _opts(max_iter=12), index_base=1) as m1:
        cuts = m1.separate_cliques(x, bases, cone=cone)
        K.assert_cliques_equal(cuts, K.restatement(X, bases, cone_idx=idx + 1), "index base 1", raw_base=1)


def test_the_handle_is_not_touched_and_refusals_leave_it_as_it_was(shapes):
    pr, mdl = shapes
    before = mdl.solve(trace_capacity=16, device_out=True)
    info = mdl.info()
    cone = SIDES.index(65)
    x = _primal(65, _gram(65))
    xd = torch.as_tensor(x, device="cuda:0")
    bases = K.bases_from_triangles(_triangles(65), 100)
    want = K.restatement(_gram(65), bases, cone_idx=_idx(65))
    K.assert_cliques_equal(mdl.separate_cliques(x, bases, cone=cone), want, "host route")
    K.assert_cliques_equal(mdl.separate_cliques(xd, bases, cone=cone, knobs=dict(batch=64)), want, "device route")
    mdl.separate_cliques(before, K.bases_from_triangles(_triangles(130), 10), cone=SIDES.index(130), min_violation=0.0)
    pent = (np.arange(5, dtype=np.int64)[None, :], np.ones((1, 5), dtype=np.int8))
    tri = (np.array([[0, 1, 2]], dtype=np.int64), np.ones((1, 3), dtype=np.int8))
    for what, b, kw, text in (("side 4, q 3", tri, dict(cone=SIDES.index(4)), "side < base_size + 2"),
                              ("side 6, q 5", pent, dict(cone=SIDES.index(6)), "side < base_size + 2"),
                              ("cone -1", tri, dict(cone=-1), "cone"), ("cone past the end", tri, dict(cone=len(SIDES)), "cone"),
                              ("node past the side", (np.array([[0, 1, 5]]), tri[1]), dict(cone=SIDES.index(5)), "outside the cone"),
                              ("not ascending", (np.array([[0, 2, 1]]), tri[1]), dict(cone=cone), "not strictly ascending"),
                              ("first sign", (tri[0], np.array([[-1, 1, 1]], dtype=np.int8)), dict(cone=cone), "first sign"),
                              ("sign", (tri[0], np.array([[1, 3, 1]], dtype=np.int8)), dict(cone=cone), "not +-1"),
                              ("knob", tri, dict(cone=cone, knobs=dict(grid=-2)), "grid")):
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.separate_cliques(xd, b, **kw)
        assert e.value.code == E_INVALID and text in str(e.value), (what, str(e.value))
    for bad in (np.nan, np.inf):
        for route in (lambda v: v, lambda v: torch.as_tensor(v, device="cuda:0")):
            y = x.copy()
            y[pr.psd[cone][1234]] = bad
            with pytest.raises(B.ProxSDPHipError) as e:
                mdl.separate_cliques(route(y), bases, cone=cone)
            assert e.value.code == E_INVALID and "non-finite" in str(e.value) and f"cone {cone}" in str(e.value)
            # a non-finite entry OUTSIDE the cone is none of this call's business
            y = x.copy()
            y[pr.psd[SIDES.index(130)][7]] = bad
            K.assert_cliques_equal(mdl.separate_cliques(route(y), bases, cone=cone), want, "outside the cone")
    with pytest.raises(ValueError):
        mdl.separate_cliques(x[:-1], bases, cone=cone)
    after = mdl.solve(trace_capacity=16, device_out=True)
    _assert_equal(after, before, "solve after the separations")
    info2 = mdl.info()
    assert info2["device_bytes"] == info["device_bytes"] and info2["updates"] == info["updates"]


# ----------------------------------------------------------------- one round past the triangles, end to end
def _tight_triangles(X, triples, patterns, tol=1e-2):
    """the triangle rows whose left side at X is within tol of 1, as bases"""
    sg = T.SIGNS[patterns]
    left = (sg[:, 0] * X[triples[:, 0], triples[:, 1]] + sg[:, 1] * X[triples[:, 0], triples[:, 2]]) + sg[:, 2] * X[triples[:, 1], triples[:, 2]]
    keep = np.abs(left - 1.0) <= tol
    return triples[keep].astype(np.int64), K.PATTERN_SIGNS[patterns[keep]]


def _round_past_the_triangles(solve0, separate_triangles, add_and_solve, separate_cliques, objective):
    """P.maxcut(60, seed=0, avg_degree=6.0), default options: four rounds of the 100 most violated triangle rows above 0.02,
    then the 50 most violated pentagonal rows grown from the tight triangles, then heptagons from those.  The CPU oracle on
    the same recipe (cold solves): objective 144.867 -> 142.490 -> 141.192 -> 140.267 -> 139.674 over the triangle rounds; 202
    of the 400 rows tight, 200 distinct pentagonal rows with violations 0.410 and below; with 50 of them the objective falls by
    0.272 to 139.402 (OPTIMAL) and the added rows keep at most 3.2e-4; the 50 pentagons grow into 50 heptagons.  The library
    with warm starts on an MI355X: 216 tight rows, 211 pentagonal rows (largest violation 0.370), objective 139.446 -> 139.199
    (a fall of 0.246), 5.0e-4 left on the added rows, 50 heptagonal rows (largest violation 0.305)."""
    r = solve0()
    assert r.status == OPTIMAL
    tri, pat = [], []
    for _ in range(4):
        cuts = separate_triangles(r)
        assert len(cuts) > 0
        tri.append(cuts.triples); pat.append(cuts.patterns)
        r = add_and_solve(r, cuts.add)
        assert r.status == OPTIMAL
    X = P.unpack_psd(_host(r.primal), 60)
    bases = _tight_triangles(X, np.concatenate(tri), np.concatenate(pat))
    assert len(bases[0]) >= 50
    five = separate_cliques(r, bases)
    K.assert_cliques_equal(five, K.restatement(X, bases, min_violation=0.02), "pentagons on the library's own X", raw_base=0)
    print(f"tight triangles {len(bases[0])}, pentagonal rows {len(five)}, largest violation {five.violations[:1]}")
    assert len(five) >= 50
    obj_before = objective(r)
    (ptr, cols, vals), h = five.add
    r5 = add_and_solve(r, ((ptr[:51], cols[:ptr[50]], vals[:ptr[50]]), h[:50]))
    assert r5.status == OPTIMAL
    X5 = P.unpack_psd(_host(r5.primal), 60)
    left = np.array([K.lhs(X5, five.nodes[q], five.signs[q]) - 2.0 for q in range(50)])
    print(f"objective {obj_before} -> {objective(r5)}, largest violation left on the added rows {left.max()}")
    assert left.max() < 0.02
    assert objective(r5) <= obj_before - 0.1
    top = (five.nodes[:50], five.signs[:50])
    seven = separate_cliques(r5, top)
    K.assert_cliques_equal(seven, K.restatement(X5, top, min_violation=0.02), "heptagons", raw_base=0)
    assert seven.size == 7 and len(seven) > 0
    whole = separate_cliques(r5, five)                               # the CliqueCuts itself as the bases
    K.assert_cliques_equal(whole, K.restatement(X5, (five.nodes, five.signs), min_violation=0.02), "heptagons from the CliqueCuts")
    print(f"heptagonal rows {len(seven)}, largest violation {seven.violations[:1]}")
    return five, seven


def test_one_round_past_the_triangles_end_to_end():
    pr = P.maxcut(60, seed=0, avg_degree=6.0)
    with B.Model(pr, _opts()) as mdl:
        def add_and_solve(prev, add):
            ch = mdl.change_rows(add=add)
            return mdl.solve(start=ch.carry(prev), device_out=True)
        five, seven = _round_past_the_triangles(
            lambda: mdl.solve(device_out=True), lambda r: mdl.separate_triangles(r, count=100, min_violation=0.02), add_and_solve,
            lambda r, bases: mdl.separate_cliques(r, bases, min_violation=0.02), lambda r: pr.user_objective(r.objval))
        assert mdl.m == 450


def test_the_optimizer_runs_the_round_on_its_kept_model():
    pr = P.maxcut(60, seed=0, avg_degree=6.0)
    opt = Optimizer()
    _round_past_the_triangles(
        lambda: opt.optimize(pr, keep_model=True), lambda r: opt.separate_triangles(r, count=100, min_violation=0.02),
        lambda prev, add: opt.reoptimize(add_rows=add, start=prev),
        lambda r, bases: opt.separate_cliques(r, bases=bases, min_violation=0.02), lambda r: r.objval)
    assert opt.problem.G.shape[0] == 450
    opt.model.close()
