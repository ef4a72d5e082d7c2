"""The start path of proxsdp_hip_solve_from on the device, through its test entry proxsdp_hip_start_point ("Init" and the
start, nothing more), against the NumPy / SciPy restatement in warm_start_cases.Internal: k_start_gather (order, sqrt(2),
D and E), the factored cones through the solver's reconstruction kernels (scalar and MFMA) straight into the iterate,
M x and M'y through the solver's product launches on the support path, the general path and with a dense A, the
target-rank rule and the step scalars.

Shapes: PSD sides 1, 2, 3, 33, 64, 65 in one model (one entry; below, at and just above the 64 x 64 reconstruction tile;
more than one tile) with an SOC cone, free variables and inequality rows, the variables not in solver order; factor
ranks 0, 1, 3 and `side` (33 and 65 columns take the MFMA kernel, a rank that is no multiple of its chunk of 16) mixed
with cones given densely; both index bases.

Bounds: x and y from dense input bit-identical (one multiply per entry; under equilibration one divide more: 2 ulp, see
_ulp_close); a factored block to 1e-14 ||X||_F (a sum of at most 65 products per entry: about sqrt(65) u relative to the
terms); M x and M'y to 1e-13 of their largest entry (rows and columns of a few hundred terms)."""
import numpy as np
import pytest

import oracle
from oracle import pdhg as opdhg
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P

from warm_start_cases import Internal, multi_block, psd_sides, random_factors, rule_target_rank

pytestmark = pytest.mark.gpu

SIDES = (1, 2, 3, 33, 64, 65)
RANKS_A = [None, 0, 3, 1, None, 3]          # 1x1 and side 64 dense; a zero block; rank = side 3; rank 1; rank 3
RANKS_B = [1, 2, None, 33, 3, 65]           # 1x1 factored; rank = side at 2, 33 and 65 (MFMA kernel from rank 16 on)
RANKS_C = [0, None, 1, 0, 64, None]         # a zero 1x1 block; rank = side at 64


def _options(**kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def _point_values(pr, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(pr.n), rng.standard_normal(pr.p), rng.standard_normal(pr.m)


def _close(got, ref, rel, what):
    scale = max(1.0, float(np.abs(ref).max())) if len(ref) else 1.0
    err = float(np.abs(got - ref).max()) if len(ref) else 0.0
    print("%s: max difference %.3e (bound %.3e)" % (what, err, rel * scale))
    assert err <= rel * scale, (what, err, rel * scale)


def _check_point(pr, I, got, primal, dual_eq, dual_in, factors, cold_x=None, x_exact=True):
    """x, y, Mx, Mty of `got` against the restatement; returns nothing, asserts"""
    x, y, Mx, Mty, blocks = I.point(primal, dual_eq, dual_in, factors, cold_x=cold_x)
    dense = np.ones(I.n, dtype=bool)
    for k, X in blocks.items():
        dense[I.off[k]:I.off[k + 1]] = False
        d = got["x"][I.off[k]:I.off[k + 1]] - x[I.off[k]:I.off[k + 1]]
        fro = float(np.linalg.norm(X))
        # (the packed form carries sqrt(2) off the diagonal: its 2-norm IS the Frobenius norm of the symmetric matrix)
        print("cone %d side %d rank %d: ||difference||_F %.3e, ||X||_F %.3e" % (k, I.sides[k], np.asarray(factors[k][0]).size,
                                                                            float(np.linalg.norm(d)), fro))
        assert np.linalg.norm(d) <= 1e-14 * fro, (k, float(np.linalg.norm(d)), fro)
    if x_exact:
        assert np.array_equal(got["x"][dense], x[dense]), "x from dense input is not bit-identical"
        assert np.array_equal(got["y"], y), "y is not bit-identical"
    _close(got["Mx"], Mx, 1e-13, "Mx")
    _close(got["Mty"], Mty, 1e-13, "Mty")
    return x, y


@pytest.fixture(scope="module")
def model():
    pr = multi_block(seed=0, sides=SIDES)
    return pr, Internal(pr)


@pytest.mark.parametrize("index_base", [0, 1])
@pytest.mark.parametrize("ranks", [RANKS_A, RANKS_B, RANKS_C], ids=["A", "B", "C"])
def test_mixed_cone_model_general_path(model, ranks, index_base):
    pr, I = model
    primal, deq, din = _point_values(pr)
    fac = random_factors(pr, ranks, seed=3)
    got = B.start_point(pr, _options(), dict(primal=primal, dual_eq=deq, dual_in=din, factors=fac), index_base=index_base)
    _check_point(pr, I, got, primal, deq, din, fac)
    assert got["iteration"] == 0
    assert list(got["target_rank"]) == list(rule_target_rank(SIDES, ranks))
    ps = got["primal_step"]
    assert abs(ps - I.cold_step) <= 1e-13 * I.cold_step and got["primal_step_old"] == ps and got["dual_step"] == ps
    o = oracle.Options()
    assert got["beta"] == o.initial_beta and got["theta"] == o.initial_theta and got["adapt_level"] == o.initial_adapt_level


def test_reconstruction_kernel_choice_does_not_change_the_point(model):
    """reconstruct_mfma = 0 / 1 force the scalar and the MFMA kernel for every factored cone, ranks below 16 and the
    rank-0 block included: the same bounds"""
    pr, I = model
    primal, deq, din = _point_values(pr, 1)
    fac = random_factors(pr, RANKS_B, seed=4)
    for mfma in (0, 1):
        got = B.start_point(pr, _options(reconstruct_mfma=mfma), dict(primal=primal, factors=fac))
        _check_point(pr, I, got, primal, None, None, fac)
        assert not got["y"].any() and not got["Mty"].any()


def test_target_rank_rule_and_the_explicit_override(model):
    pr, I = model
    fac = random_factors(pr, RANKS_A, seed=5)
    explicit = [5, 0, 2, 0, 9, 70]                                    # capped at sides 1 and 65; 0 = derive
    got = B.start_point(pr, _options(), dict(factors=fac, target_rank=explicit))
    assert list(got["target_rank"]) == list(rule_target_rank(SIDES, RANKS_A, explicit)) == [1, 2, 2, 2, 9, 65]
    got = B.start_point(pr, _options(initial_target_rank=4), dict(factors=fac))
    assert list(got["target_rank"]) == list(rule_target_rank(SIDES, RANKS_A, initial=4)) == [1, 2, 3, 4, 4, 4]
    # without factors the explicit ranks still hold, and a start that gives no point leaves the cold vectors alone
    cold = B.start_point(pr, _options(), None)
    got = B.start_point(pr, _options(), dict(target_rank=explicit))
    assert list(got["target_rank"]) == [1, 2, 2, 2, 9, 65] and list(cold["target_rank"]) == [1, 2, 2, 2, 2, 2]
    for k in ("x", "y", "Mx", "Mty"):
        assert np.array_equal(got[k], cold[k]), k
    assert not cold["Mx"].any() and not cold["y"].any()               # (a cold solve has (M x)_old = 0, x = tau c)
    assert np.allclose(cold["x"], cold["primal_step"] * I.c, rtol=1e-15, atol=0)
    empty = B.start_point(pr, _options(), {})
    for k in ("x", "y", "Mx", "Mty", "target_rank"):
        assert np.array_equal(empty[k], cold[k]), k


def test_partial_starts_keep_the_cold_values_elsewhere(model):
    """primal = NULL: every variable outside a factored cone keeps tau c (advanced_initialization) or 0; duals only: x = the
    cold x and M x is computed from it"""
    pr, I = model
    _, deq, din = _point_values(pr, 2)
    fac = random_factors(pr, RANKS_A, seed=6)
    for adv in (1, 0):
        o = _options(advanced_initialization=adv)
        cold = B.start_point(pr, o, None)
        assert adv == 1 or not cold["x"].any()
        got = B.start_point(pr, o, dict(factors=fac, dual_in=din))
        _check_point(pr, I, got, None, None, din, fac, cold_x=cold["x"])
        got = B.start_point(pr, o, dict(dual_eq=deq))
        _check_point(pr, I, got, None, deq, None, None, cold_x=cold["x"])
        assert list(got["target_rank"]) == list(cold["target_rank"])


def test_given_primal_step_and_beta(model):
    pr, I = model
    primal, deq, din = _point_values(pr, 3)
    got = B.start_point(pr, _options(), dict(primal=primal, dual_eq=deq, primal_step=0.125, beta=3.5))
    assert got["primal_step"] == 0.125 and got["primal_step_old"] == 0.125 and got["dual_step"] == 0.125 and got["beta"] == 3.5
    _check_point(pr, I, got, primal, deq, None, None)
    got = B.start_point(pr, _options(), dict(beta=0.5))               # the scalars hold without a point as well
    assert got["beta"] == 0.5 and abs(got["primal_step"] - I.cold_step) <= 1e-13 * I.cold_step


def test_exact_norm_step(model):
    """approx_norm = 0: the cold step is 1 / sigma_max(M)"""
    pr, I = model
    primal, deq, din = _point_values(pr, 4)
    got = B.start_point(pr, _options(approx_norm=0), dict(primal=primal, dual_eq=deq, dual_in=din))
    smax = float(np.linalg.svd(I.M.toarray(), compute_uv=False)[0])
    assert abs(got["primal_step"] - 1.0 / smax) <= 1e-10 / smax, (got["primal_step"], 1.0 / smax)
    _check_point(pr, I, got, primal, deq, din, None)


@pytest.mark.parametrize("support_path", [0, 1])
def test_psd_only_model_on_both_vector_paths(support_path):
    """no SOC and no 1x1 block, so that support_path = 1 is legal; the objective only on the diagonals and few entries per
    row: the support is a strict subset of the variables (M'y lives on it in the support path's compact buffer)"""
    sides = (2, 3, 33, 64, 65)
    pr = multi_block(seed=1, sides=sides, soc_len=0, density=0.01, diag_c=True)
    I = Internal(pr)
    supp = (np.diff(I.M.tocsc().indptr) > 0) | (I.c != 0)
    assert 0.2 * pr.n < supp.sum() < 0.6 * pr.n
    primal, deq, din = _point_values(pr, 5)
    ranks = [2, None, 33, 1, 65]
    fac = random_factors(pr, ranks, seed=7)
    o = _options(support_path=support_path)
    got = B.start_point(pr, o, dict(primal=primal, dual_eq=deq, dual_in=din, factors=fac))
    _check_point(pr, I, got, primal, deq, din, fac)
    assert list(got["target_rank"]) == list(rule_target_rank(sides, ranks))
    assert not got["Mty"][~supp].any()
    cold = B.start_point(pr, o, None)
    got = B.start_point(pr, o, dict(factors=fac, dual_eq=deq))
    _check_point(pr, I, got, None, deq, None, fac, cold_x=cold["x"])


def _ulp_close(got, num, den, ulps, what):
    """|got - num / den| <= ulps ulp with den known to one rounding (den = a long double): see _probe_scaling"""
    ref = (np.asarray(num, np.longdouble) / den)
    err = np.abs(np.asarray(got, np.longdouble) - ref)
    worst = float(np.max(err / np.spacing(np.abs(got)))) if len(got) else 0.0
    print("%s: worst difference %.2f ulp" % (what, worst))
    assert np.all(err <= ulps * np.spacing(np.abs(got))), (what, worst)


def _probe_scaling(pr, I0, o):
    """The library's equilibration diagonals, read through the start path itself: the point (1, ..., 1) comes back as
    s / D and 1 / E, each ONE rounding away from the true quotient, so in extended precision D~ = s / x and E~ = 1 / y
    carry a relative error of at most u.  A second point p then has to come back as fl(fl(p s) / D): within u of the true
    quotient, which is within u of fl(p s) / D~ -- 2 u <= 2 ulp in all."""
    one = B.start_point(pr, o, dict(primal=np.ones(pr.n), dual_eq=np.ones(pr.p), dual_in=np.ones(pr.m)))
    s = np.where(I0.offdiag, np.sqrt(2.0), 1.0)
    return s.astype(np.longdouble) / one["x"].astype(np.longdouble), np.longdouble(1.0) / one["y"].astype(np.longdouble)


def test_forced_equilibration(model):
    """x = primal s / D, y = dual / E: one divide more per entry, 2 ulp; the factored blocks take lambda / d"""
    pr, I0 = model
    o = _options(equilibration_force=1)
    Dl, El = _probe_scaling(pr, I0, o)
    # they ARE the equilibration diagonals: the oracle's equilibrate! on the reordered [A;G]
    aff, cones = oracle.api.to_standard_form(pr)
    opdhg.preprocess(aff, cones)
    import scipy.sparse as sp
    Eo, Do = opdhg.equilibrate(sp.vstack([aff.A, aff.G], format="csc"), aff, oracle.Options())
    assert np.allclose(np.asarray(Dl, float), Do, rtol=1e-9) and np.allclose(np.asarray(El, float), Eo, rtol=1e-9)
    assert np.ptp(np.asarray(Dl, float)) <= 4e-16 * float(Dl[0])       # D = d I
    I = Internal(pr, np.asarray(El, float), np.asarray(Dl, float))
    primal, deq, din = _point_values(pr, 6)
    fac = random_factors(pr, RANKS_B, seed=8)
    got = B.start_point(pr, o, dict(primal=primal, dual_eq=deq, dual_in=din, factors=fac))
    _check_point(pr, I, got, primal, deq, din, fac, x_exact=False)
    dense = np.ones(I.n, dtype=bool)
    for k, r in enumerate(RANKS_B):
        if r is not None:
            dense[I.off[k]:I.off[k + 1]] = False
    num = np.where(I.offdiag, primal[I.ord] * np.sqrt(2.0), primal[I.ord])
    _ulp_close(got["x"][dense], num[dense], Dl[dense], 2, "x")
    _ulp_close(got["y"], np.concatenate([deq, din]), El, 2, "y")
    assert abs(got["primal_step"] - I.cold_step) <= 1e-12 * I.cold_step


@pytest.mark.parametrize("equil", [0, 1])
def test_dense_constraint_matrix(equil):
    """randsdp n = 12, m = 8 with a dense A (and the sparse variable bounds in G): M x through the dense product kernels,
    with their scale vectors when equilibrated, M'y through the dense transposed product"""
    pr = P.randsdp(12, 8, seed=2, dense=True)
    o = _options(equilibration_force=equil)
    E, D, fro, _, eq = B.dense_scaling(pr, o)
    assert eq == bool(equil)
    I = Internal(pr, E, D) if equil else Internal(pr)
    assert abs(fro - 1.0 / I.cold_step) <= 1e-12 * fro
    primal, deq, din = _point_values(pr, 7)
    for fac in (None, [(np.array([1.5, 0.25, 2.0]), np.random.default_rng(9).standard_normal((12, 3)) / 3.0)]):
        got = B.start_point(pr, o, dict(primal=primal, dual_eq=deq, dual_in=din, factors=fac))
        _check_point(pr, I, got, primal, deq, din, fac, x_exact=not equil)
        if equil and fac is None:
            num = np.where(I.offdiag, primal[I.ord] * np.sqrt(2.0), primal[I.ord])
            _ulp_close(got["x"], num, D.astype(np.longdouble), 2, "x")
            _ulp_close(got["y"], np.concatenate([deq, din]), E.astype(np.longdouble), 2, "y")
        assert list(got["target_rank"]) == [2 if fac is None else 4]
    got = B.start_point(pr, _options(equilibration_force=equil, approx_norm=0), dict(primal=primal))
    smax = float(np.linalg.svd(I.M.toarray(), compute_uv=False)[0])
    assert abs(got["primal_step"] - 1.0 / smax) <= 1e-10 / smax
