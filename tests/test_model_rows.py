"""Inequality rows added to and dropped from a model handle on the GPU (proxsdp_hip_model_rows, csrc/model_rows.hip.hpp,
binding.Model.change_rows): after a change the handle IS a fresh model of the changed problem -- its dump equals the fresh
model's dump and its solve equals the fresh proxsdp_hip_solve_device call bit for bit.  "Equal" is test_model_handle.py's:
np.array_equal / == on the six vectors, the trace without its wall-clock column, iter, status, final_rank, the objectives,
the gap, the residuals, the factors and every integer counter of stats.  Long solves are capped with max_iter."""
import numpy as np
import pytest
import scipy.sparse as sp

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

import kat_problems as K
import model_rows_cases as R

pytestmark = pytest.mark.gpu

VECTORS = ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in")
SCALARS = ("status", "certificate_found", "primal_feasible_user_tol", "dual_feasible_user_tol", "result_count", "final_rank",
           "iter", "primal_residual", "dual_residual", "objval", "dual_objval", "gap", "dual_feasibility", "status_string")
INT_STATS = tuple(k for k, t in B.Stats._fields_ if t is B.i64) + ("reserved_s",)
TRACE_ELAPSED = 12
CAP = 48
E_INVALID, E_UNSUPP = -1, -4
SIDE96 = dict(min_size_krylov_eigs=32, max_iter=40)
MIXED = dict(max_iter=120)


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


def _assert_dumps_equal(a, b, what, norms_equal=True):
    for k, _ in B.MODEL_DUMP_ARRAYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("n", "Q", "nnz", "ns"):
        assert a[k] == b[k], (what, k)
    if norms_equal:
        for k in B.MODEL_NORM_NAMES:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _fresh(pr, okw, **skw):
    return B.solve(pr, _opts(**okw), trace_capacity=CAP, device_out=True, factors=True, **skw)


def _on_model(mdl, **skw):
    return mdl.solve(trace_capacity=CAP, device_out=True, factors=True, **skw)


def _maxcut96():
    return P.maxcut(96, seed=0, avg_degree=6.0)


def _changed(pr, add=None, drop=None):
    G2, h2, kept, _ = R.stack_rows(pr.G, pr.h, add, drop)
    return R.with_rows(pr, G2, h2), kept


def _assert_is_fresh_model(mdl, pr2, okw, what, **skw):
    """dump and solve of the handle against a fresh model / a fresh solve of pr2; returns the handle's result"""
    with B.Model(pr2, _opts(**okw)) as ref:
        got, exp = mdl.dump(), ref.dump()
        assert np.array_equal(got["support"], exp["support"]) and got["ns"] == exp["ns"], (what, "support")
        _assert_dumps_equal(got, exp, what)
        assert mdl.info()["use_support"] == ref.info()["use_support"], what
    res = _on_model(mdl, **skw)
    _assert_equal(res, _fresh(pr2, okw, **skw), what)
    return res


# ----------------------------------------------------------------- 1. known answer, m from 0 up
def test_the_five_cycle_with_all_its_triangle_rows_has_the_cut_value():
    """C5 has no K5 minor, so its metric polytope is its cut polytope: with all 40 triangle rows the relaxation is exact
    (max cut 4); without them it gives 5 (1 + cos(pi / 5)) / 2 = 4.52254.  The CPU oracle, default options: 4.523947 after 42
    iterations and 3.9999995 after 41; the band 5e-3 separates 4.52 from 4.00 and sits above both deviations."""
    import oracle
    pr = R.c5()
    add = R.triangle_rows(5, R.all_triples(5))
    pr2, kept = _changed(pr, add)
    assert pr2.G.shape == (40, 15)
    with B.Model(pr, _opts()) as mdl:
        r0 = _on_model(mdl)
        _assert_equal(r0, _fresh(pr, {}), "C5")
        print("C5", pr.user_objective(r0.objval), r0.iter)
        assert abs(pr.user_objective(r0.objval) - 5.0 * (1.0 + np.cos(np.pi / 5.0)) / 2.0) <= 5e-3
        ch = mdl.change_rows(add=add)
        assert ch.m == 40 and np.array_equal(ch.kept, kept) and mdl.m == 40
        r1 = _assert_is_fresh_model(mdl, pr2, {}, "C5 with 40 triangle rows")
        print("C5 + triangles", pr2.user_objective(r1.objval), r1.iter)
        assert abs(pr2.user_objective(r1.objval) - 4.0) <= 5e-3
    for p_, r_ in ((pr, r0), (pr2, r1)):
        ref = oracle.api.solve(p_, oracle.Options())
        assert r_.status == ref.status == 1
        got = p_.user_objective(r_.objval)                         # (the oracle returns the user's sense)
        assert abs(got - ref.objval) <= 1e-9 * (1 + abs(ref.objval)), (got, ref.objval)


# ----------------------------------------------------------------- 2. support path, rebuild
def test_triangle_rows_on_the_support_path_rebuild_the_support_and_leave_again():
    pr = _maxcut96()
    add = R.triangle_rows(96, R.first_triples(96, 3))
    pr2, _ = _changed(pr, add)
    first = _fresh(pr, SIDE96)
    with B.Model(pr, _opts(**SIDE96)) as mdl, B.Model(pr, _opts(**SIDE96)) as orig:
        d0 = orig.dump()
        ch = mdl.change_rows(add=add)
        assert (ch.m, ch.nnz, ch.support_rebuilt) == (12, 96 + 36, 1)
        info = mdl.info()
        assert info["support_rebuilds"] == 1 and info["m"] == 12 and info["use_support"] == 1
        res = _assert_is_fresh_model(mdl, pr2, SIDE96, "12 triangle rows")
        assert res.stats["fop_projections"] > 0 and res.stats["cycle_launches"] > 0
        ch = mdl.change_rows(drop=np.arange(12))
        assert ch.m == 0 and len(ch.kept) == 0 and mdl.info()["m"] == 0
        _assert_dumps_equal(mdl.dump(), d0, "rows dropped again")
        back = _on_model(mdl)
        _assert_equal(back, first, "rows dropped again")
        assert back.stats["fop_projections"] > 0 and back.stats["cycle_launches"] > 0


# ----------------------------------------------------------------- 3. more than one workgroup
def test_two_hundred_triangle_rows_span_several_workgroups():
    pr = _maxcut96()
    add = R.triangle_rows(96, R.first_triples(96, 50))
    pr2, _ = _changed(pr, add)
    with B.Model(pr, _opts(**SIDE96)) as mdl:
        ch = mdl.change_rows(add=add)
        assert ch.m == 200 and ch.nnz == 696 and ch.nnz > 2 * 256 and ch.nnz % 256 != 0
        _assert_is_fresh_model(mdl, pr2, SIDE96, "200 triangle rows")


# ----------------------------------------------------------------- 4. general path with existing rows
def _mixed_rows(pr):
    """4 new rows over the free and SOC variables and one diagonal PSD entry of K.mixed_cones()"""
    in_cone = np.zeros(pr.n, dtype=bool)
    for idx in list(pr.psd) + list(pr.soc):
        in_cone[idx] = True
    free = np.flatnonzero(~in_cone)
    soc = pr.soc[0]
    diag = int(pr.psd[2][0])                                    # entry (0, 0) of the side-104 block
    cols = np.array([free[0], soc[1], free[1], soc[0], diag, free[2], soc[2], soc[3], free[0]], dtype=np.int64)
    ptr = np.array([0, 2, 5, 6, 9], dtype=np.int64)
    vals = np.array([0.5, -1.25, 1.0, 0.25, 0.75, -2.0, 1.5, -0.5, 0.125])
    return (ptr, cols, vals), np.array([3.0, 4.0, 5.0, 6.0])


def test_drop_and_add_in_one_call_on_the_general_path_then_a_value_update():
    pr = K.mixed_cones()
    add = _mixed_rows(pr)
    pr2, kept = _changed(pr, add, [1, 5, 11])
    assert list(kept) == [0, 2, 3, 4, 6, 7, 8, 9, 10, -1, -1, -1, -1]
    with B.Model(pr, _opts(**MIXED)) as mdl:
        ch = mdl.change_rows(add=add, drop=[11, 1, 5])
        assert np.array_equal(ch.kept, kept) and ch.m == 13 and ch.support_rebuilt == 0
        _assert_is_fresh_model(mdl, pr2, MIXED, "drop 3, add 4")
        rng = np.random.default_rng(4)
        G3 = sp.csc_matrix(pr2.G)
        G3.data = G3.data * (1.0 + 0.01 * rng.choice([-1.0, 1.0], size=len(G3.data)))
        mdl.update(G_values=G3.data)
        _assert_is_fresh_model(mdl, R.with_rows(pr2, G3, pr2.h), MIXED, "values in the new storage order")


# ----------------------------------------------------------------- 5. down to m' = 0 and back
def test_every_row_dropped_and_added_back_in_another_order():
    pr = K.sdp_wiki(False)
    G = sp.csr_matrix(pr.G)
    order = [2, 0, 3, 1]
    with B.Model(pr, _opts()) as mdl:
        _assert_equal(_on_model(mdl), _fresh(pr, {}), "before")
        ch = mdl.change_rows(drop=[3, 2, 1, 0])
        assert ch.m == 0
        pr0, _ = _changed(pr, None, range(4))
        _assert_is_fresh_model(mdl, pr0, {}, "no inequality row")
        ch = mdl.change_rows(add=(G[order, :], pr.h[order]))
        assert ch.m == 4 and list(ch.kept) == [-1] * 4
        pr4 = R.with_rows(pr, sp.csc_matrix(G[order, :]), pr.h[order])
        _assert_is_fresh_model(mdl, pr4, {}, "the rows in another order")


# ----------------------------------------------------------------- 6. warm start across a change
def test_a_warm_start_carried_across_a_change_equals_the_fresh_warm_solve():
    import torch
    pr = _maxcut96()
    add = R.triangle_rows(96, R.first_triples(96, 3))
    pr2, kept = _changed(pr, add)
    with B.Model(pr, _opts(**SIDE96)) as mdl:
        prev = _on_model(mdl)
        ch = mdl.change_rows(add=add)
        start = ch.carry(prev)
        assert torch.is_tensor(start["dual_in"]) and start["dual_in"].is_cuda and start["primal"] is prev.primal
        assert start["dual_in"].shape == (12,) and not bool(start["dual_in"].any())
        res = _on_model(mdl, start=start)
        _assert_equal(res, _fresh(pr2, SIDE96, start=start), "device start carried")
        host_prev = dict(primal=_host(prev.primal), dual_eq=_host(prev.dual_eq), dual_in=_host(prev.dual_in))
        hstart = ch.carry(host_prev)
        assert isinstance(hstart["dual_in"], np.ndarray) and np.array_equal(hstart["dual_in"], np.zeros(12))
        _assert_equal(_on_model(mdl, start=hstart), _fresh(pr2, SIDE96, start=hstart), "host start carried")
        # a second change on the same handle, now with duals to carry: equal on the kept rows, zero on the new ones
        add3 = R.triangle_rows(96, [(5, 40, 77)])
        pr3, kept3 = _changed(pr2, add3, [1, 6])
        ch = mdl.change_rows(add=add3, drop=[1, 6])
        start3 = ch.carry(res)
        d_old, d_new = _host(res.dual_in), _host(start3["dual_in"])
        assert start3["dual_in"].is_cuda and np.array_equal(ch.kept, kept3)
        assert len(d_new) == 14 and np.array_equal(d_new[:10], d_old[kept3[:10]]) and np.all(d_new[10:] == 0.0)
        _assert_equal(_on_model(mdl, start=start3), _fresh(pr3, SIDE96, start=start3), "second change, device start")
        h3 = ch.carry(dict(dual_in=d_old))
        assert isinstance(h3["dual_in"], np.ndarray) and np.array_equal(h3["dual_in"], d_new)


# ----------------------------------------------------------------- 7. device route
def test_device_route_of_integer_rows_equals_the_host_route():
    """Integer-valued new rows on columns whose factor is 1 (diagonal PSD entries) with integer h: every square and every
    partial sum is an integer far below 2^53, exact in any order, so the device route's norms equal the host's."""
    import torch
    pr = _maxcut96()
    rng = np.random.default_rng(3)
    k = 37
    ptr = np.arange(0, 3 * k + 1, 3, dtype=np.int64)
    cols = np.concatenate([P.tri_index(d, d) for d in (rng.choice(96, size=3, replace=False) for _ in range(k))]).astype(np.int64)
    vals = rng.integers(1, 9, size=3 * k).astype(float)
    h_new = rng.integers(20, 40, size=k).astype(float)
    cuda = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    with B.Model(pr, _opts(**SIDE96)) as mh, B.Model(pr, _opts(**SIDE96)) as md:
        ch_h = mh.change_rows(add=((ptr, cols, vals), h_new))
        ch_d = md.change_rows(add=((cuda(ptr).long(), cuda(cols).long(), cuda(vals)), cuda(h_new)))
        assert ch_h.support_rebuilt == 0 and ch_d.support_rebuilt == 0 and ch_d.m == k
        _assert_dumps_equal(md.dump(), mh.dump(), "integer rows")
        _assert_equal(_on_model(md), _on_model(mh), "integer rows")


def test_device_route_of_triangle_rows_agrees_in_the_norms_and_equals_elsewhere():
    """4 eps sqrt(len) relative: a random-walk estimate of the rounding of a sum of len squares, not its worst case (the
    factor sqrt(2)/2 enters the squares)"""
    import torch
    pr = _maxcut96()
    (ptr, cols, vals), h_new = R.triangle_rows(96, R.first_triples(96, 50))
    vals = vals * 1.1
    h_new = h_new * 0.9
    cuda = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    with B.Model(pr, _opts(**SIDE96)) as mh, B.Model(pr, _opts(**SIDE96)) as md:
        mh.change_rows(add=((ptr, cols, vals), h_new))
        md.change_rows(add=((ptr, cols, cuda(vals)), cuda(h_new)))
        dh, dd = mh.dump(), md.dump()
        _assert_dumps_equal(dd, dh, "triangle rows", norms_equal=False)
        assert dd["norm_b"] == dh["norm_b"] and dd["norm_c"] == dh["norm_c"]
        for name, ln in (("norm_h", len(h_new)), ("frob", dh["nnz"])):
            print(name, dh[name], dd[name], abs(dh[name] - dd[name]) / dh[name])
            assert abs(dh[name] - dd[name]) <= 4 * np.finfo(float).eps * np.sqrt(ln) * abs(dh[name]), name


# ----------------------------------------------------------------- 8. failure leaves the handle whole
def test_refused_changes_leave_the_handle_whole():
    import torch
    pr = K.mixed_cones()
    want = _fresh(pr, MIXED)
    (ptr, cols, vals), h_new = _mixed_rows(pr)
    cuda = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    bad_vals = vals.copy()
    bad_vals[4] = np.nan
    bad_cols = cols.copy()
    bad_cols[2] = pr.n
    refused = {
        "non-finite device value": (dict(add=((ptr, cols, cuda(bad_vals)), cuda(h_new))), "add_val"),
        "non-finite device h": (dict(add=((ptr, cols, cuda(vals)), cuda(np.array([1.0, np.inf, 0.0, 0.0])))), "add_h"),
        "column out of range": (dict(add=((ptr, bad_cols, vals), h_new)), "column out of range"),
        "repeated drop": (dict(drop=[2, 7, 2]), "repeated"),
    }
    with B.Model(pr, _opts(**MIXED)) as mdl:
        before = mdl.dump()
        for name, (kw, text) in refused.items():
            bytes0 = mdl.info()["device_bytes"]
            with pytest.raises(B.ProxSDPHipError) as e:
                mdl.change_rows(**kw)
            assert e.value.code == E_INVALID and text in str(e.value), (name, str(e.value))
            assert mdl.m == 12 and mdl.info()["m"] == 12 and mdl.info()["device_bytes"] == bytes0
            _assert_dumps_equal(mdl.dump(), before, name)
            _assert_equal(_on_model(mdl), want, name)
        assert mdl.info()["support_rebuilds"] == 0


@pytest.mark.parametrize("okw", [dict(equilibration_force=1), dict(approx_norm=0)], ids=["equilibrated", "exact_norm"])
def test_models_whose_set_up_depends_on_the_rows_refuse_and_repeat_their_solves(okw):
    pr = K.sdp_wiki(False)
    want = _fresh(pr, okw)
    with B.Model(pr, _opts(**okw)) as mdl:
        _assert_equal(_on_model(mdl), want, 0)
        with pytest.raises(B.ProxSDPHipError) as e:
            mdl.change_rows(drop=[0])
        assert e.value.code == E_UNSUPP
        assert mdl.m == 4
        _assert_equal(_on_model(mdl), want, 1)


# ----------------------------------------------------------------- 9. not a rebuild
def test_a_change_allocates_less_than_the_model_and_leaks_nothing_per_round():
    pr = _maxcut96()
    add = R.triangle_rows(96, R.first_triples(96, 3))
    with B.Model(pr, _opts(**SIDE96)) as mdl:
        whole = mdl.info()["device_bytes"]
        ch = mdl.change_rows(add=add)
        print("bytes_allocated", ch.bytes_allocated, "of", whole)
        assert 0 < ch.bytes_allocated < whole                     # (a full re-create would allocate at least `whole`)
        after_first = mdl.info()["device_bytes"]
        mdl.change_rows(drop=np.arange(12))
        mdl.change_rows(add=add)
        assert mdl.info()["device_bytes"] == after_first
        mdl.change_rows(drop=np.arange(12))
        mdl.change_rows(add=add)
        assert mdl.info()["device_bytes"] == after_first
    with pytest.raises(ValueError):
        mdl.info()
    with B.Model(pr, _opts(**SIDE96)) as again:
        assert again.info()["device_bytes"] == whole


# ----------------------------------------------------------------- 10. across the long-row limit of M x
SIDE130 = dict(min_size_krylov_eigs=32, max_iter=30)


def _full_rows(n, count, parts=1):
    """`count` rows with an entry in every one of the n columns -- small integers, so every stored value, product with 1.0 and
    sum of squares of unscaled values is exact -- each cut into `parts` consecutive pieces (rows of their own); h = 40000 is
    above 3 n |x| for every x the first iterations reach: the rows are slack"""
    ptr, cols, vals = [0], [], []
    for r in range(count):
        for piece in np.array_split(np.arange(n, dtype=np.int64), parts):
            cols += piece.tolist()
            vals += (1.0 + (piece + r) % 3).tolist()
            ptr.append(len(cols))
    return (np.array(ptr, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals)), np.full(len(ptr) - 1, 40000.0)


def test_a_row_longer_than_the_segment_limit_comes_and_goes():
    """Side 130 has 8515 variables, the smallest side above the 8192 entries from which M x takes a row in segments
    (Solver::LONG_ROW): a row over every column switches the segmented launches on, dropping it switches them off, two such
    rows give two long rows.  After every step the handle is a fresh model of the changed problem, and after the drop it holds
    the bytes it held before the add: the segment buffers went with the last long row.  Before that comparison the handle is
    warmed with the same entries in two half rows (none above the limit), solved and dropped again: the staging buffer of host
    values only grows (it is sized by the largest change so far), and a solve allocates some workspaces on first use; neither
    is what the comparison is about."""
    pr = P.maxcut(130, seed=0, avg_degree=6.0)
    assert pr.n == 130 * 131 // 2 == 8515 and pr.n > 8192 and pr.G.shape[0] == 0
    one, two, halves = _full_rows(pr.n, 1), _full_rows(pr.n, 2), _full_rows(pr.n, 1, parts=2)
    assert np.diff(halves[0][0]).max() <= 8192 < np.diff(one[0][0]).min()
    with B.Model(pr, _opts(**SIDE130)) as mdl:
        mdl.change_rows(add=halves)
        _assert_is_fresh_model(mdl, _changed(pr, halves)[0], SIDE130, "two half rows")
        mdl.change_rows(drop=[0, 1])
        before = mdl.info()["device_bytes"]
        ch = mdl.change_rows(add=one)
        assert (ch.m, ch.nnz) == (1, 130 + pr.n)
        print("device_bytes", before, "with the long row", mdl.info()["device_bytes"])
        _assert_is_fresh_model(mdl, _changed(pr, one)[0], SIDE130, "one long row")
        ch = mdl.change_rows(drop=[0])
        assert (ch.m, ch.nnz) == (0, 130)
        after = mdl.info()["device_bytes"]
        print("device_bytes after the drop", after)
        _assert_is_fresh_model(mdl, pr, SIDE130, "long row dropped")
        assert after == before, (after, before)
        ch = mdl.change_rows(add=two)
        assert (ch.m, ch.nnz) == (2, 130 + 2 * pr.n)
        _assert_is_fresh_model(mdl, _changed(pr, two)[0], SIDE130, "two long rows")


# ----------------------------------------------------------------- 11. Optimizer
def _assert_same_sol(a, b, what):
    for k in ("status", "iter", "objval", "dual_objval", "gap", "final_rank"):
        assert getattr(a, k) == getattr(b, k), (what, k, getattr(a, k), getattr(b, k))
    for k in VECTORS:
        assert np.array_equal(_host(getattr(a, k)), _host(getattr(b, k))), (what, k)


@pytest.mark.parametrize("max_sense", [False, True])
def test_reoptimize_with_new_rows_equals_optimize_of_the_changed_problem(max_sense):
    pr = K.sdp_wiki(max_sense)
    # -0.9 <= X4 <= 0.8 cuts off both optima (-0.978 and 0.872)
    add = ((np.array([0, 1, 2]), np.array([3, 3]), np.array([1.0, -1.0])), np.array([0.8, 0.9]))
    pr2, _ = _changed(pr, add)
    kept = Optimizer()
    s0 = kept.optimize(pr, keep_model=True)
    s1 = kept.reoptimize(add_rows=add, start=s0)
    assert kept.problem.G.shape == (6, 6) and np.array_equal(kept.problem.h, pr2.h)
    assert (sp.csc_matrix(kept.problem.G) != sp.csc_matrix(pr2.G)).nnz == 0
    carried = B.start_from_result(s0)
    carried["dual_in"] = np.concatenate([carried["dual_in"], np.zeros(2)])
    p1 = Optimizer().optimize(pr2, start=carried)
    _assert_same_sol(s1, p1, "reoptimize(add_rows=...)")
    assert kept.objective_value() == p1.objval
    exp = 0.8 if max_sense else -0.9
    assert abs(kept.objective_value() - exp) <= 1e-2, kept.objective_value()
    # a later reoptimize(h=...) sees the new shape; dropping the new rows gives the first problem again
    s2 = kept.reoptimize(h=pr2.h)
    _assert_same_sol(s2, Optimizer().optimize(pr2), "reoptimize(h=...) after the change")
    s3 = kept.reoptimize(drop_rows=[4, 5])
    _assert_same_sol(s3, Optimizer().optimize(pr), "rows dropped again")
    kept.model.close()
