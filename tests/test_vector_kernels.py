"""The linesearch's production kernels and the cone tail against exact references (vector_kernel_cases.py), through
proxsdp_hip_trial_batch / proxsdp_hip_cone_tail, which run the solver's own launches (k_dual_trial_batch, both
instantiations of k_spmvT_batch with the wave-per-long-column sums and of k_residual_xy -- <false> on the general path,
<true> on the support path --, k_combine_multi, k_primal_update_S; k_soc_project, k_soc_gap, k_clamp_scalars).

y+ and M'y+ of every candidate and the six maxima are compared with `==` on bits: the element-wise expressions are compiled
without contraction, the column sums are specified in storage order, a maximum has no order.  The five sums are compared
with math.fsum under the any-order bound 2 N 2^-53 sum|terms| (vector_kernel_cases.sum_bound)."""
import math

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import vector_kernel_cases as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert B.device_count() > 0, "no HIP device: the product path has no CPU fallback"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero(_bits(got).ravel() != _bits(exp).ravel())[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {got.size} differ, first at flat index {bad[0]}: "
                           f"{got.ravel()[bad[0]]!r} != {exp.ravel()[bad[0]]!r}")


def _check_scalars(got, maxs, sums, slots, what):
    for q in slots:
        if q in maxs:
            assert got[q] == maxs[q], (what, q, got[q], maxs[q])
            continue
        t = sums[q]
        if len(t) and not np.all(np.isfinite(t)):
            # an infinite h: inf * y is +-inf or NaN for every y, in any order (the reference's dot gives the same)
            with np.errstate(invalid="ignore"):
                exp = float(np.sum(t))
            assert (math.isnan(exp) and math.isnan(got[q])) or got[q] == exp, (what, q, got[q], exp)
            continue
        exact, bound = math.fsum(t), V.sum_bound(t)
        print(f"{what} slot {q}: |got - fsum| = {abs(got[q] - exact):.3e}, bound {bound:.3e}")
        assert abs(got[q] - exact) <= bound, (what, q, got[q], exact, bound)


def _run(cs, nc=3, **kw):
    """one batch on the GPU against the reference; returns the hook's output"""
    out = B.trial_batch(cs["colptr"], cs["row"], cs["val"], cs["Q"], **V.hook_args(cs, nc=nc, **kw))
    ref = V.reference(cs, nc=nc, **kw)
    what = f"{cs['name']} nc={nc} {kw}"
    cap = lambda L: min(V.PSTRIDE, max(1, -(-L // V.TPB)))
    assert out["gq"] == cap(cs["Q"]) and out["gx"] == cap(len(ref["S"])), (what, out["gq"], out["gx"])
    if kw.get("support"):
        assert np.array_equal(out["supp"], ref["S"]), what
        _same_bits(out["x_upd"], ref["x_upd"], what + " k_primal_update_S x")
        _same_bits(out["xsave"], ref["xsave"], what + " xsave")
        _same_bits(out["esv"], ref["esv"], what + " esv")
    for k in range(nc):
        _same_bits(out["y"][k], ref["y"][k], f"{what} y+ of candidate {k}")
    for k in range(nc):
        _same_bits(out["Mty"][k], ref["Mty"][k], f"{what} M'y+ of candidate {k}")
    for k in range(nc):
        _check_scalars(out["scal"][k], ref["maxs"][k], ref["sums"][k], range(V.NSCAL), f"{what} candidate {k}")
    if kw.get("c0", -1) >= 0:
        _check_scalars(out["scal_re"], ref["re"][0], ref["re"][1], range(2, V.NSCAL), what + " re-evaluation")
    return out


# ----------------------------------------------------------------- vector lengths around one wave and one workgroup
@pytest.mark.parametrize("pkind", [0, 1, 2], ids=["p0", "pQ", "pmixed"])
@pytest.mark.parametrize("size", [1, 63, 64, 65, 255, 256, 257])
def test_batch_at_small_lengths(size, pkind):
    cs = V.small_case(size, pkind)
    _run(cs, support=False)
    _run(cs, support=True, tau_update=0.21)
    _run(cs, support=bool(pkind % 2), plain=True, tau_update=0.4)


# ----------------------------------------------------------------- batch width, re-evaluation, special values
@pytest.mark.parametrize("support", [False, True], ids=["general", "support"])
@pytest.mark.parametrize("nc", [1, 2, 3])
def test_batch_width_and_reevaluation_leg(nc, support):
    cs = V.special_case("plain")
    _run(cs, nc=nc, support=support, tau_update=0.3)
    # residuals(t1, 1, c) of linesearch_and_residuals: the last candidate again, with steps of its own
    _run(cs, nc=nc, support=support, c0=nc - 1, tau_re=0.0771, sigma_re=0.0533, tau_update=0.3)
    if nc == 3:
        _run(cs, nc=nc, support=support, c0=1, tau_re=0.0771, sigma_re=0.0533)


@pytest.mark.parametrize("support", [False, True], ids=["general", "support"])
@pytest.mark.parametrize("kind", ["slack", "ties", "inf", "roww", "xold0"])
def test_batch_special_values(kind, support):
    """slack: every Mx - h < 0, so max(Mx - h) must be exactly +0.0;  ties: ybar / bt == h exactly;  roww: zero weights on
    some rows;  xold0: x_old = 0 at k = 1;  inf: h = +inf on five rows -- y+ and every other scalar are finite and exact there,
    but h'y itself cannot be: inf * y is +-inf or NaN for every y (0 * inf included), in the reference's dot as well, so that
    one slot is compared as the non-finite value the terms give in any order."""
    cs = V.special_case(kind)
    for plain in (False, True):
        out = _run(cs, support=support, plain=plain, tau_update=0.3)
        if kind == "slack":
            assert np.all(out["scal"][:, 8] == 0.0) and not np.signbit(out["scal"][:, 8]).any()


# ----------------------------------------------------------------- long columns: lengths and placements
@pytest.mark.parametrize("plain", [False, True], ids=["linesearch", "plain"])
def test_column_lengths_and_placements_general_path(plain):
    _run(V.column_case(), plain=plain)


@pytest.mark.parametrize("plain", [False, True], ids=["linesearch", "plain"])
def test_column_lengths_and_placements_support_order(plain):
    cs = V.column_case()
    _run(V.embed(cs, V.column_keep(cs["n"])), support=True, plain=plain, tau_update=0.3)


# ----------------------------------------------------------------- past the grid cap: the grid-stride loops
@pytest.fixture(scope="module")
def capped():
    return V.capped_case()


def test_grid_stride_general_path(capped):
    out = _run(capped, support=False)
    assert capped["Q"] > out["gq"] * V.TPB and capped["n"] > out["gx"] * V.TPB       # the loops really ran twice


def test_grid_stride_support_order(capped):
    w = V.embed(capped, V.capped_keep(capped["n"]))
    out = _run(w, support=True, tau_update=0.3)
    assert w["Q"] > out["gq"] * V.TPB and len(out["supp"]) > out["gx"] * V.TPB


# ----------------------------------------------------------------- the column map is the only difference between the paths
@pytest.mark.parametrize("cs", V.identity_support_cases(), ids=lambda cs: cs["name"])
def test_identity_support_is_the_general_path(cs):
    """a support that holds every column: the support path's y+, M'y+ and all 11 scalars are the general path's bits"""
    for plain in (False, True):
        gen = _run(cs, nc=3, support=False, plain=plain)
        sup = _run(cs, nc=3, support=True, plain=plain)
        assert np.array_equal(sup["supp"], np.arange(cs["n"]))
        what = f"{cs['name']} plain={plain}: support path against general path,"
        _same_bits(sup["y"], gen["y"], what + " y+")
        _same_bits(sup["Mty"], gen["Mty"], what + " M'y+")
        _same_bits(sup["scal"], gen["scal"], what + " scalars")


def test_transposed_spmv_entry_runs_the_production_kernel():
    """proxsdp_hip_spmv(transpose=1) is k_spmvT_batch<false> with one plain candidate: bits of the storage-order loop
    (binding.spmv sorts the rows of a column, so storage order is ascending rows here)"""
    import scipy.sparse as sp
    cs = V.column_case()
    M = sp.csc_matrix((cs["val"], cs["row"], cs["colptr"]), shape=(cs["Q"], cs["n"]))
    M.sort_indices()
    y = np.random.default_rng(3).standard_normal(cs["Q"])
    exp = V.col_dots(M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data, y)[0]
    _same_bits(B.spmv(M, y, transpose=True), exp, "spmv transpose")


# ----------------------------------------------------------------- second-order cones and 1x1 blocks
@pytest.fixture(scope="module")
def cone_run():
    x, off, ln, one_off, cases = V.soc_layout()
    return x, off, ln, one_off, cases, B.cone_tail(x, off, ln, one_off)


def test_soc_projection_branches_ties_and_lengths(cone_run):
    """Every cone of one launch against the longdouble reference.  The tie nv == s needs no case of its own beyond
    (5, 3, 4): there the scaling branch computes val = 0.5 (1 + s / nv) = 1 exactly and returns the same bits, so `<=` and `<`
    cannot be told apart by any input.  The tie nv == -s can: scaling by val = 0 leaves -0.0 where the tail is negative, the
    polar branch writes +0.0 (case tie_3_m4_m5)."""
    x, off, ln, one_off, cases, (x_soc, g0, g1, x_cl, me) = cone_run
    inside = np.zeros(len(x), dtype=bool)
    for ci, ((name, branch, v), o, L) in enumerate(zip(cases, off, ln)):
        inside[o:o + L] = True
        got = x_soc[o:o + L]
        _, exp, nv, gap = V.soc_reference(v)
        bound = V.soc_bound(L, v[0], nv)
        if branch == "inside":
            _same_bits(got, v, name)                                    # untouched, bit for bit
        elif branch == "polar":
            _same_bits(got, np.zeros(L), name)                          # +0.0 everywhere (also from s = -0.0)
        else:
            err = float(np.max(np.abs(got.astype(np.longdouble) - exp)))
            print(f"{name}: max error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (name, err, bound)
        assert abs(float(np.longdouble(g0[ci]) - gap)) <= bound, (name, g0[ci], float(gap))
        assert g1[ci] <= bound, (name, g1[ci], bound)                    # the projected point is in the cone
    _same_bits(x_soc[~inside], x[~inside], "entries outside every cone")


def test_soc_projection_is_idempotent(cone_run):
    x, off, ln, one_off, cases, (x_soc, g0, g1, x_cl, me) = cone_run
    again = B.cone_tail(x_soc, off, ln, np.zeros(0, dtype=np.int64))[0]
    for (name, branch, v), o, L in zip(cases, off, ln):
        _, _, nv, _ = V.soc_reference(v)
        d = float(np.max(np.abs(again[o:o + L] - x_soc[o:o + L])))
        assert d <= V.soc_bound(L, v[0], nv), (name, d)
        if branch != "outside":
            _same_bits(again[o:o + L], x_soc[o:o + L], name + " twice")


def test_clamp_scalars_at_scattered_offsets(cone_run):
    x, off, ln, one_off, cases, (x_soc, g0, g1, x_cl, me) = cone_run
    exp = x_soc.copy()
    exp[one_off] = np.maximum(0.0, x[one_off])
    assert np.array_equal(x_cl, exp)
    assert np.array_equal(me, exp[one_off]) and np.all(me >= 0.0)
    rest = np.ones(len(x), dtype=bool)
    rest[one_off] = False
    _same_bits(x_cl[rest], x_soc[rest], "entries that are no 1x1 block")
