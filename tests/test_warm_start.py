"""Warm-started solves (proxsdp_hip_solve_from through binding.solve(..., start=...) and the layers above it): a solve
entered from a previous solution's factors and duals stops as early as the loop allows, follows the CPU oracle resumed
from the same point, and serves every model class and vector path.

Iteration caps come from the oracle (tests/test_warm_start_host.py measures the rule; oracle runs with reference defaults: Max-Cut n = 150
seed 0 cold 2741 iterations, 41 = min_iter + 1 from its own factors at target rank rank + 1, 202 at target rank rank,
2774 at the cold default of 2; sensorloc n = 20 cold 11533, warm 1006), with room for a different stop on a chaotic tail:
a tenth resp. a fifth of the cold count.  Objectives of a solve and its restart from its own result: within
2 tol_gap (1 + |objval|); where a start is only partial, or the model changed, _stops_agree's bound."""
import numpy as np
import pytest

import oracle
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import moi
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

from kat_problems import sdp_plus_soc, sdp_wiki, soc_norm
from test_solution_factors import block, check_cone
from warm_start_cases import Internal, oracle_state0, rule_target_rank

pytestmark = pytest.mark.gpu

TOL_GAP = oracle.Options().tol_gap
MIN_ITER = oracle.Options().min_iter
TRACE_ELAPSED = 12                                  # trace column 12 is wall-clock time: the one column two runs do not share


def _obj_close(a, b):
    return abs(a - b) <= 2.0 * TOL_GAP * (1.0 + abs(b))


def _stops_agree(s1, s2):
    """For starts that are only partial and for a changed model: two solves of one model that both stop OPTIMAL have |p - d| <= tol_gap (1 + |p| + |d|)
    each, and p and d bracket the optimum (up to the feasibility tolerance), so their primal objectives differ by at most
    tol_gap (2 + |p1| + |d1| + |p2| + |d2|) -- about twice _obj_close's bound, which a start far from the dual solution
    (primal only: y = 0) does use up."""
    return abs(s1.objval - s2.objval) <= TOL_GAP * (2.0 + abs(s1.objval) + abs(s1.dual_objval) + abs(s2.objval) + abs(s2.dual_objval))


@pytest.fixture(scope="module")
def maxcut150():
    """Max-Cut n = 150 seed 0, reference defaults (Krylov path, one-workgroup cycle kernel): the cold solve with its factors"""
    pr = P.maxcut(150, seed=0)
    cold = Optimizer().optimize(pr, trace_capacity=8000, factors=True)
    assert cold.status == 1 and cold.trace.shape[0] == cold.iter
    info = cold.psd_factors[0][2]
    assert info["rank"] == info["rank_found"] > 0
    warm = Optimizer().optimize(pr, trace_capacity=8000, start=cold)
    return pr, cold, warm


def test_maxcut_from_its_own_factors_and_duals(maxcut150):
    pr, cold, warm = maxcut150
    rank = cold.psd_factors[0][2]["rank_found"]
    print("cold %d iterations (rank %d), warm %d; objective %.9g / %.9g" % (cold.iter, rank, warm.iter, cold.objval, warm.objval))
    assert warm.status == 1
    assert int(warm.trace[0][0]) == 1 and int(warm.trace[0][10]) == rank + 1
    assert 10 * warm.iter <= cold.iter, (warm.iter, cold.iter)
    assert _obj_close(warm.objval, cold.objval)
    assert warm.stats["cycle_launches"] > 0 and warm.stats["lanczos_matvecs"] > 0          # the Krylov path served it


def test_warm_solve_follows_the_oracle_resumed_from_the_same_point(maxcut150):
    """the same user-unit arrays through oracle.chambolle_pock(resume=state0): iteration 0, zero history, cold scalars,
    target rank by the rule.  Iteration count, target-rank column and linesearch trials equal; trace columns to
    1e-8 max(1, |t|), the bound test_state_seam.py applies to library-versus-oracle continuations."""
    pr, cold, warm = maxcut150
    vals, vecs, info = cold.psd_factors[0]
    I = Internal(pr)
    x, y, Mx, Mty, _ = I.point(cold.primal, cold.dual_eq, cold.dual_in, [(vals, vecs)])
    o = oracle.Options()
    tr = rule_target_rank([150], [info["rank"]])
    ora = oracle.solve(pr, o, trace=True, resume=oracle_state0(x, y, Mx, Mty, tr, o, I.cold_step))
    print("oracle %d iterations, library %d" % (ora.iter, warm.iter))
    assert ora.status == warm.status == 1 and ora.iter == warm.iter
    lt = {int(r[0]): r for r in warm.trace}
    worst = 0.0
    for t in ora.trace:
        r = lt[t["iter"]]
        assert int(r[10]) == t["target_rank"][0] and int(r[11]) == t["trials"], (t["iter"], r[10], r[11], t["target_rank"], t["trials"])
        for col, key in ((1, "prim_obj"), (2, "dual_obj"), (3, "gap"), (4, "feas"), (7, "primal_step"), (8, "beta")):
            d = abs(r[col] - t[key]) / max(1.0, abs(t[key]))
            worst = max(worst, d)
            assert d <= 1e-8, (t["iter"], key, r[col], t[key])
    print("worst trace difference %.3e" % worst)
    assert abs(warm.objval - ora.objval) <= 1e-8 * max(1.0, abs(ora.objval))


def test_dense_primal_start_with_the_factored_runs_target_rank(maxcut150):
    pr, cold, warm = maxcut150
    rank = cold.psd_factors[0][2]["rank_found"]
    st = dict(primal=cold.primal, dual_eq=cold.dual_eq, dual_in=cold.dual_in, target_rank=[rank + 1])
    dense = Optimizer().optimize(pr, trace_capacity=8000, start=st)
    assert dense.status == 1 and dense.iter == warm.iter and int(dense.trace[0][10]) == rank + 1
    assert abs(dense.objval - warm.objval) <= 1e-8 * abs(warm.objval)
    # without the target rank the point alone does not pay: the first projection truncates it to the cold default of 2
    assert Optimizer(max_iter=10 * warm.iter).optimize(pr, start=dict(st, target_rank=None)).status == 3


def test_partial_and_empty_starts(maxcut150):
    pr, cold, warm = maxcut150
    rank = cold.psd_factors[0][2]["rank_found"]
    duals = Optimizer().optimize(pr, start=dict(dual_eq=cold.dual_eq, dual_in=cold.dual_in))
    primal = Optimizer().optimize(pr, start=dict(factors=[cold.psd_factors[0][:2]]), trace_capacity=1)
    print("duals only: %d iterations, primal (factors) only: %d, cold %d" % (duals.iter, primal.iter, cold.iter))
    assert duals.status == 1 and _stops_agree(duals, cold)
    assert primal.status == 1 and _stops_agree(primal, cold) and int(primal.trace[0][10]) == rank + 1
    # a start with every field NULL is the cold solve, bit for bit
    empty = Optimizer().optimize(pr, trace_capacity=8000, start={})
    assert empty.iter == cold.iter and empty.objval == cold.objval and np.array_equal(empty.primal, cold.primal)
    keep = [c for c in range(B.TRACE_COLS) if c != TRACE_ELAPSED]
    assert np.array_equal(empty.trace[:, keep], cold.trace[:, keep])


def test_chained_warm_solves_hand_their_factors_on(maxcut150):
    pr, cold, warm = maxcut150
    w1 = Optimizer().optimize(pr, start=cold, factors=True)
    assert w1.status == 1 and w1.iter == warm.iter and w1.objval == warm.objval          # (fac changes nothing of the solve)
    check_cone("warm maxcut150", block(w1.primal, pr, 0), w1.psd_factors[0])
    info = w1.psd_factors[0][2]
    assert info["rank"] == info["rank_found"] == cold.psd_factors[0][2]["rank_found"]
    w2 = Optimizer().optimize(pr, start=w1, factors=True)
    assert w2.status == 1 and w2.iter == MIN_ITER + 1, w2.iter
    assert _obj_close(w2.objval, cold.objval)


def _sensorloc():
    return P.sensorloc(20, seed=0), {}


def _equilibrated_kat():
    return sdp_wiki(False), dict(equilibration_force=1)


def _dense_randsdp():
    # (chosen with the oracle among small instances: cold 1969 iterations, restarted from its own result 59, objectives
    # 1.5 % of the bound apart; randsdp instances whose cold stop is loose -- n = 5, m = 5, seed 1: 73 % -- are no test)
    return P.randsdp(6, 4, seed=1, varbounds=True, dense=True), {}


CLASSES = {
    "soc_norm": (lambda: (soc_norm(), {}), 1.0),
    "sdp_plus_soc": (lambda: (sdp_plus_soc(), {}), 1.0),
    "sensorloc20": (_sensorloc, 0.2),
    "mimo40": (lambda: (P.mimo(40, seed=0), {}), 1.0),                # small-block sign kernel
    "equilibrated_kat": (_equilibrated_kat, 1.0),
    "dense_randsdp": (_dense_randsdp, 1.0),
}


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_other_model_classes_from_their_own_cold_result(name):
    build, share = CLASSES[name]
    pr, kw = build()
    cold = Optimizer(**kw).optimize(pr, factors=True)
    warm = Optimizer(**kw).optimize(pr, start=cold)
    print("%s: cold %d iterations, warm %d; objective %.9g / %.9g" % (name, cold.iter, warm.iter, cold.objval, warm.objval))
    assert cold.status == 1 and warm.status == 1
    assert warm.iter <= share * cold.iter, (warm.iter, cold.iter)
    assert _obj_close(warm.objval, cold.objval)
    if name == "mimo40":
        assert warm.stats["batched_small_eigs"] > 0
    if name == "dense_randsdp":
        assert warm.stats["dense_passes"] > 0


@pytest.mark.parametrize("support_path", [0, 1])
def test_both_vector_paths(support_path):
    """Max-Cut n = 150 again with the vector path forced either way (support_path = 1: the operator-form Lanczos mat-vec
    from the second iteration on; the first projection reads the packed start)"""
    pr = P.maxcut(150, seed=0)
    cold = Optimizer(support_path=support_path).optimize(pr, factors=True)
    warm = Optimizer(support_path=support_path).optimize(pr, start=cold)
    print("support_path %d: cold %d iterations, warm %d" % (support_path, cold.iter, warm.iter))
    assert warm.status == 1 and 10 * warm.iter <= cold.iter and _obj_close(warm.objval, cold.objval)
    assert (warm.stats["fop_projections"] > 0) == bool(support_path)


def _readme_maxcut(W):
    """the README's Max-Cut model (max 0.25 <W, X>, diag X = 1, X PSD) through the model layer"""
    m = moi.Model()
    X = m.add_variables(10)
    m.add_constraint(moi.VectorOfVariables(X), moi.PositiveSemidefiniteConeTriangle(4))
    V = moi.ivech(X)
    for i in range(4):
        m.add_constraint(moi.ScalarAffineFunction([moi.ScalarAffineTerm(1.0, int(V[i, i]))], 0.0), moi.EqualTo(1.0))
    _set_objective(m, V, W)
    return m, V


def _set_objective(m, V, W):
    terms = [moi.ScalarAffineTerm(0.25 * (W[i, j] if i == j else 2.0 * W[i, j]), int(V[i, j])) for j in range(4) for i in range(j + 1)]
    m.set_objective_sense(moi.MAX_SENSE)
    m.set_objective_function(moi.ScalarAffineFunction(terms, 0.0))


def test_model_layer_warm_start_after_an_objective_change():
    W0 = P.README_W
    W1 = W0.copy()
    W1[0, 1] = W1[1, 0] = -5.5                                        # one edge weight changes, and the degrees with it
    W1[0, 0] += 0.5; W1[1, 1] += 0.5
    m, V = _readme_maxcut(W0)
    first = m.optimize(warm=True)                                     # nothing to start from yet: a cold solve, factors kept
    assert first.status == 1 and m.start_values(warm=True) is not None
    _set_objective(m, V, W1)
    for i in range(4):
        m.set_variable_primal_start(int(V[i, i]), 1.0)                # what the constraints pin
    warm = m.optimize(warm=True)
    ref, _ = _readme_maxcut(W1)
    cold = ref.optimize()
    print("objective change: cold %d iterations, warm %d; objective %.9g / %.9g" % (cold.iter, warm.iter, cold.objval, warm.objval))
    assert warm.status == 1 and cold.status == 1 and warm.iter < cold.iter
    assert _stops_agree(warm, cold)                                   # the NEW optimum, not the one it started from
    assert abs(first.objval - cold.objval) > 10 * TOL_GAP * (1.0 + abs(cold.objval))
    assert m.objective_value() == warm.objval
