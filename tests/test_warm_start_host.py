"""CPU-only tests of the warm start's boundary (proxsdp_hip_solve_from, proxsdp_hip_start_point, proxsdp_start): the ctypes
structure and the Julia shim list the header's members in order, every malformed proxsdp_start is rejected on the host --
before a solver, and with it a device, exists (this machine has none: a call that got as far as the device would come back
with PROXSDP_E_HIP) --, the Python layers marshal a start correctly, and the rule the library derives a target rank by is
pinned with the CPU oracle."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import moi
from proxsdp_jl_amd import problems as P

from kat_problems import mixed_cones, sdp_wiki
from test_host_abi import _c_struct_fields
from warm_start_cases import Internal, oracle_state0, oracle_warm, rule_target_rank

NEW_FUNCTIONS = ("proxsdp_hip_solve_from", "proxsdp_hip_start_point")


def test_start_struct_mirrors_the_header_field_by_field():
    header = B.HEADER_PATH.read_text()
    cf = _c_struct_fields(header, "proxsdp_start")
    assert [f for f, _ in B.Start._fields_] == cf
    assert C.sizeof(B.Start) == 8 * len(cf) == 104                   # thirteen 8-byte members, no padding
    jl = (B.HEADER_PATH.parent.parent / "julia" / "ProxSDPHip.jl").read_text()
    body = re.search(r"struct Start\b.*?\n(.*?)\nend", jl, re.S).group(1)
    jf = [re.match(r"\s*(\w+)::", ln).group(1) for ln in body.splitlines() if re.match(r"\s*\w+::", ln)]
    assert jf == cf
    assert ":proxsdp_hip_solve_from" in jl


def test_new_functions_are_exported_and_the_abi_version_stays():
    L = B.lib()
    names = set(B.header_symbols())
    for f in NEW_FUNCTIONS:
        assert f in names, f"{f} is not declared in include/proxsdp_hip.h"
        assert hasattr(L, f), f"{f} is not exported"
    assert L.proxsdp_hip_abi_version() == 10


# ----------------------------------------------------------------- argument errors, straight through the C ABI
def _wiki_start():
    """a well-formed start for sdp_wiki (one PSD cone of side 3, 3 equalities, inequality rows): everything given"""
    pr = sdp_wiki(False)
    rng = np.random.default_rng(0)
    V = rng.standard_normal((3, 2))
    st = dict(primal=rng.standard_normal(pr.n), dual_eq=rng.standard_normal(pr.p), dual_in=rng.standard_normal(pr.m),
              factors=[(np.array([2.0, 0.5]), V)], target_rank=[0], primal_step=0.25, beta=2.0)
    return pr, st


def _call(entry, mutate):
    """`entry` on sdp_wiki with a well-formed proxsdp_start that `mutate` then damages"""
    L = B.lib()
    pr, st = _wiki_start()
    M = B._Marshalled(pr)
    o = B.default_options()
    S, arr = B._start_struct(pr.n, pr.p, pr.m, B.psd_sides(pr), st)
    mutate(S, arr, M)
    if entry == "solve_from":
        R = B.Result()
        rc = L.proxsdp_hip_solve_from(C.byref(M.P), C.byref(o), C.byref(R), C.byref(S), None)
    else:
        T, tarr = B._state_struct(pr.n, pr.p + pr.m, 1, o.convergence_window)
        rc = L.proxsdp_hip_start_point(C.byref(M.P), C.byref(o), C.byref(S), C.byref(T))
    return rc, L.proxsdp_hip_last_error().decode()


def _set(field, value):
    def m(S, arr, M):
        setattr(S, field, value)
    return m


def _arr(name, index, value):
    def m(S, arr, M):
        arr[name][index] = value
    return m


INVALID = {
    "struct_size": _set("struct_size", 8),
    "n_psd_mismatch": _set("n_psd", 2),
    "null_rank": _set("rank", None),
    "null_vec_ptr": _set("vec_ptr", None),
    "null_val_ptr": _set("val_ptr", None),
    "rank_below_minus_one": _arr("rank", 0, -2),
    "rank_above_side": _arr("rank", 0, 4),
    "vec_span_too_small": _arr("vec_ptr", 1, 3 * 2 - 1),
    "val_span_too_small": _arr("val_ptr", 1, 1),
    "null_vectors": _set("vectors", None),
    "null_values": _set("values", None),
    "nan_primal": _arr("primal", 2, np.nan),
    "inf_dual_eq": _arr("dual_eq", 1, np.inf),
    "nan_dual_in": _arr("dual_in", 0, np.nan),
    "inf_vector": _arr("vectors", 4, -np.inf),
    "nan_value": _arr("values", 1, np.nan),
    "zero_value": _arr("values", 0, 0.0),
    "negative_value": _arr("values", 1, -1.0),
    "negative_target_rank": _arr("target_rank", 0, -1),
    "negative_primal_step": _set("primal_step", -1.0),
    "nan_primal_step": _set("primal_step", float("nan")),
    "negative_beta": _set("beta", -0.5),
}


@pytest.mark.parametrize("entry", ["solve_from", "start_point"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_malformed_start_is_rejected_before_touching_the_device(case, entry):
    rc, msg = _call(entry, INVALID[case])
    assert rc == -1, (case, rc, msg)                                 # PROXSDP_E_INVALID, not PROXSDP_E_HIP
    assert msg


def _shard_reduce_fn(S, arr, M):
    cb = B.REDUCE_FN(lambda ctx, ps, ns, pm, nm: 0)
    M.keep.append(cb)
    M.P.reduce_fn = C.cast(cb, C.c_void_p)


def _shard_reduce_vec_fn(S, arr, M):
    cb = B.REDUCE_VEC_FN(lambda ctx, ptr, ln, dev: 0)
    M.keep.append(cb)
    M.P.reduce_vec_fn = C.cast(cb, C.c_void_p)


def _shard_comm(S, arr, M):
    M.P.nccl_comm = C.c_void_p(0x1000)                               # (never dereferenced: refused on the host)


def _shard_coupling(S, arr, M):
    M.P.n_coupling = 1


@pytest.mark.parametrize("entry", ["solve_from", "start_point"])
@pytest.mark.parametrize("mutate", [_shard_reduce_fn, _shard_reduce_vec_fn, _shard_comm, _shard_coupling],
                         ids=["reduce_fn", "reduce_vec_fn", "nccl_comm", "n_coupling"])
def test_a_shard_is_refused_on_the_host(mutate, entry):
    rc, msg = _call(entry, mutate)
    assert rc == -4 and "shard" in msg, (rc, msg)                    # PROXSDP_E_UNSUPP


@pytest.mark.parametrize("entry", ["solve_from", "start_point"])
def test_well_formed_start_reaches_the_device(entry):
    """the control of the cases above: the unharmed struct passes the host checks (without a GPU the call then fails
    with PROXSDP_E_HIP, with one it runs)"""
    rc, msg = _call(entry, lambda S, arr, M: None)
    assert rc == (0 if B.device_count() > 0 else -2), msg


def test_a_malformed_factors_struct_beside_a_start_is_rejected_too():
    L = B.lib()
    pr, st = _wiki_start()
    M = B._Marshalled(pr)
    o = B.default_options()
    S, arr = B._start_struct(pr.n, pr.p, pr.m, [3], st)
    F, farr = B._factors_struct([3], True)
    F.rank = None
    R = B.Result()
    assert L.proxsdp_hip_solve_from(C.byref(M.P), C.byref(o), C.byref(R), C.byref(S), C.byref(F)) == -1


# ----------------------------------------------------------------- marshalling
class _FakeLib:
    """records the entry points binding.solve calls; every call succeeds"""

    def __init__(self):
        self.calls, self.starts = [], []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            if name == "proxsdp_hip_solve_from":                     # (the arrays behind the struct live only during the call)
                S, n = args[3]._obj, args[0]._obj.n
                self.starts.append(dict(struct_size=S.struct_size, n_psd=S.n_psd, primal_step=S.primal_step, beta=S.beta,
                                        rank=S.rank[0], vec_ptr=S.vec_ptr[1], val_ptr=S.val_ptr[1], target_rank=S.target_rank[0],
                                        values=[S.values[k] for k in range(2)], vectors=[S.vectors[k] for k in range(6)],
                                        primal=[S.primal[k] for k in range(n)]))
            return 0
        return f


def test_start_none_marshals_to_the_plain_calls(monkeypatch):
    fake = _FakeLib()
    o = B.default_options()
    monkeypatch.setattr(B, "lib", lambda: fake)
    pr, st = _wiki_start()
    B.solve(pr, o)
    B.solve(pr, o, start=None)
    B.solve(pr, o, start=None, factors=True)
    assert [c[0] for c in fake.calls] == ["proxsdp_hip_solve", "proxsdp_hip_solve", "proxsdp_hip_solve_factored"]
    fake.calls.clear()
    B.solve(pr, o, start=st)
    B.solve(pr, o, start=st, factors=True)
    assert [c[0] for c in fake.calls] == ["proxsdp_hip_solve_from", "proxsdp_hip_solve_from"]
    assert fake.calls[0][1][4] is None and fake.calls[1][1][4] is not None
    S = fake.starts[0]
    assert S["struct_size"] == C.sizeof(B.Start) and S["n_psd"] == 1 and S["primal_step"] == 0.25 and S["beta"] == 2.0
    assert S["rank"] == 2 and S["vec_ptr"] == 6 and S["val_ptr"] == 2 and S["target_rank"] == 0
    assert S["values"] == [2.0, 0.5]
    V = st["factors"][0][1]
    assert S["vectors"] == list(V[:, 0]) + list(V[:, 1])             # column-major, ld = side
    assert S["primal"] == list(st["primal"])
    for bad in (dict(resume={}), dict(capture_iteration=3), dict(reduce=lambda s, m: None), dict(nccl_comm=1),
                dict(coupling=dict(rows=[0], owned=[1]))):
        with pytest.raises(ValueError):
            B.solve(pr, o, start=st, **bad)


def test_start_struct_of_a_partial_start_leaves_the_rest_null():
    S, arr = B._start_struct(6, 3, 2, [3], dict(dual_eq=[1.0, 2.0, 3.0]))
    assert not S.primal and not S.dual_in and S.n_psd == 0 and not S.rank and not S.target_rank
    assert S.primal_step == 0.0 and S.beta == 0.0 and [S.dual_eq[k] for k in range(3)] == [1.0, 2.0, 3.0]
    S, arr = B._start_struct(6, 3, 2, [3], {})
    assert not S.primal and not S.dual_eq and not S.dual_in and S.n_psd == 0
    S, arr = B._start_struct(7, 0, 0, [3, 1], dict(factors=[None, (np.zeros(0), np.zeros((1, 0)))]))
    assert S.n_psd == 2 and list(arr["rank"]) == [-1, 0] and list(arr["vec_ptr"]) == [0, 0, 0]
    for bad in (dict(primal=np.zeros(5)), dict(dual_in=np.zeros(3)), dict(factors=[None, None]), dict(target_rank=[1, 2]),
                dict(factors=[(np.ones(2), np.ones((3, 1)))]), dict(x=np.zeros(6))):
        with pytest.raises(ValueError):
            B._start_struct(6, 3, 2, [3], bad)


def _result(primal, dual_eq, dual_in, factors=None):
    r = object.__new__(B.SolveResult)
    r.primal, r.dual_eq, r.dual_in = primal, dual_eq, dual_in
    if factors is not None:
        r.psd_factors = factors
    return r


def test_a_previous_result_becomes_a_start_and_a_cone_cut_by_cap_falls_back_to_its_primal_entries():
    rng = np.random.default_rng(1)
    x, ye, yi = rng.standard_normal(9), rng.standard_normal(2), rng.standard_normal(1)
    V0, V1 = rng.standard_normal((3, 2)), rng.standard_normal((2, 1))
    info = lambda rank, found, cap: dict(rank=rank, rank_found=found, cap=cap, source=1, resid=0.0, xnorm=1.0)
    res = _result(x, ye, yi, [(np.array([3.0, 1.0]), V0, info(2, 2, 3)), (np.array([2.0]), V1, info(1, 2, 1))])
    d = B.start_from_result(res)
    assert np.array_equal(d["primal"], x) and np.array_equal(d["dual_eq"], ye) and np.array_equal(d["dual_in"], yi)
    assert d["factors"][1] is None                                   # rank_found 2 > rank 1: cut by cap
    assert np.array_equal(d["factors"][0][0], [3.0, 1.0]) and np.array_equal(d["factors"][0][1], V0)
    S, arr = B._start_struct(9, 2, 1, [3, 2], res)                   # the result itself is accepted
    assert list(arr["rank"]) == [2, -1] and list(arr["vec_ptr"]) == [0, 6, 6] and list(arr["val_ptr"]) == [0, 2, 2]
    # no factors in the result: primal and duals only
    d = B.start_from_result(_result(x, ye, yi))
    assert "factors" not in d
    S, arr = B._start_struct(9, 2, 1, [3, 2], _result(x, ye, yi))
    assert S.n_psd == 0 and bool(S.primal)
    # a cone that asked for no factors (cap 0) falls back as well; without a primal that cannot work
    res = _result(None, ye, yi, [(np.array([3.0, 1.0]), V0, info(2, 2, 3)), (np.zeros(0), np.zeros((2, 0)), info(0, 0, 0))])
    with pytest.raises(ValueError):
        B.start_from_result(res)
    res.psd_factors[1] = (np.zeros(0), np.zeros((2, 0)), info(0, 0, 2))       # a complete rank-0 factor is a zero block
    d = B.start_from_result(res)
    assert d["primal"] is None and d["factors"][1][1].shape == (2, 0)


def test_model_layer_start_values():
    """VariablePrimalStart / ConstraintDualStart go through the inverse of the getters' maps, and optimize(warm=True)
    reuses the last raw result only while n, p, m and the cones are unchanged"""
    m = moi.Model()
    X = m.add_variables(3)
    t = m.add_variable()
    m.add_constraint(moi.VectorOfVariables(X), moi.PositiveSemidefiniteConeTriangle(2))
    ceq = m.add_constraint(moi.ScalarAffineFunction([moi.ScalarAffineTerm(1.0, X[0])], 0.0), moi.EqualTo(1.0))
    cge = m.add_constraint(moi.ScalarAffineFunction([moi.ScalarAffineTerm(1.0, t)], 0.0), moi.GreaterThan(-2.0))
    cle = m.add_constraint(moi.ScalarAffineFunction([moi.ScalarAffineTerm(1.0, t)], 0.0), moi.LessThan(5.0))
    assert m.start_values() is None and m.start_values(warm=True) is None
    m.set_variable_primal_start(t, 0.5)
    m.set_constraint_dual_start(ceq, 3.0)
    m.set_constraint_dual_start(cge, 0.25)
    m.set_constraint_dual_start(cle, -0.75)
    assert m.variable_primal_start(t) == 0.5 and m.variable_primal_start(X[0]) is None
    assert m.constraint_dual_start(ceq) == 3.0 and m.constraint_dual_start(cge) == 0.25 and m.constraint_dual_start(cle) == -0.75
    st = m.start_values()
    assert list(st["primal"]) == [0.0, 0.0, 0.0, 0.5]
    # constraint_dual returns flip * -(row dual): the library's row duals are the inverse of that
    assert list(st["dual_eq"]) == [-3.0] and list(st["dual_in"]) == [0.25, 0.75]
    with pytest.raises(TypeError):
        m.set_constraint_dual_start(moi.ConstraintIndex("psd", 1), 1.0)
    # warm: the last raw result, overlaid with the start values; its factors dropped for a cone with a start value
    rng = np.random.default_rng(2)
    last = _result(rng.standard_normal(4), np.array([7.0]), np.array([1.0, 2.0]),
                   [(np.array([1.5]), rng.standard_normal((2, 1)), dict(rank=1, rank_found=1, cap=2))])
    m._last = (m._shape(), last)
    st = m.start_values(warm=True)
    assert st["primal"][3] == 0.5 and np.array_equal(st["primal"][:3], last.primal[:3]) and st["factors"][0] is not None
    assert list(st["dual_eq"]) == [-3.0] and list(st["dual_in"]) == [0.25, 0.75]
    m.set_variable_primal_start(X[1], 0.1)
    assert m.start_values(warm=True)["factors"][0] is None
    m.set_variable_primal_start(X[1], None)
    m.set_constraint_dual_start(ceq, None)
    assert list(m.start_values(warm=True)["dual_eq"]) == [7.0]
    m.add_variable()                                                 # the model changed shape: the old result is not reused
    st = m.start_values(warm=True)
    assert "factors" not in st and len(st["primal"]) == 5 and "dual_eq" not in st


# ----------------------------------------------------------------- the rule, pinned with the CPU oracle
def test_target_rank_rule():
    assert list(rule_target_rank([1, 2, 3, 40], [-1, 0, 3, 5])) == [1, 2, 3, 6]
    assert list(rule_target_rank([1, 2, 3, 40], None, explicit=[0, 9, 1, 7])) == [1, 2, 1, 7]
    assert list(rule_target_rank([40, 40], [1, None], initial=4)) == [4, 4]


def test_oracle_restarted_from_its_own_result_stops_at_once_only_at_rank_plus_one():
    """Max-Cut n = 60, seed 1.  The oracle, resumed at iteration 0 from its own cold result in user units (the restatement
    of the library's start path), stops OPTIMAL at min_iter + 1 when the target rank is rank + 1 -- the projection sees the
    first non-positive eigenvalue and the rank test passes at once -- and needs more than a convergence window when the
    target rank is the rank itself: why proxsdp_hip_solve_from derives rank + 1.
    The target rank only acts on a block that takes the Krylov branch (side > min_size_krylov_eigs, reference default
    100): at side 60 under the defaults every projection is a full_eig! and ANY target rank stops at min_iter + 1
    (measured: 41 / 41 / 41 for rank + 1 / rank / 2).  So the two restarts below run with min_size_krylov_eigs = 50,
    which puts the side-60 block on the Krylov branch (measured: 41 and 202 iterations; 1414 at target rank 2); the cold
    solve they start from is the reference-default one (464 iterations, rank 5)."""
    pr = P.maxcut(60, seed=1)
    opt = oracle.Options()
    cold = oracle.solve(pr, opt)
    assert cold.status == 1
    rank = int(cold.final_rank)
    X = P.unpack_psd(cold.primal[pr.psd[0]], 60)
    assert int(np.sum(np.linalg.eigvalsh(X) > 1e-6 * np.linalg.norm(X))) == rank
    default = oracle_warm(pr, cold, [rank + 1], opt)                 # reference defaults: full_eig!, stops at once
    assert default.status == 1 and default.iter == opt.min_iter + 1, (default.status, default.iter)
    kry = oracle.Options()
    kry.min_size_krylov_eigs = 50
    warm = oracle_warm(pr, cold, [rank + 1], kry)
    print("cold %d iterations, rank %d; restart at rank + 1: %d, at rank: " % (cold.iter, rank, warm.iter), end="")
    assert warm.status == 1 and warm.iter == kry.min_iter + 1, (warm.status, warm.iter)
    assert abs(warm.objval - cold.objval) <= 2 * opt.tol_gap * (1 + abs(cold.objval))
    same = oracle_warm(pr, cold, [rank], kry)
    print(same.iter)
    assert same.status == 1 and same.iter > kry.convergence_window, (same.status, same.iter)
    assert cold.iter > 10 * warm.iter


def test_restatement_of_the_start_point_inverts_the_exit_path():
    """Internal.point applied to an oracle result reproduces the oracle's own final internal iterate to rounding"""
    pr = mixed_cones(seed=2, sides=(1, 3, 12, 2), soc_len=3, nfree=2, p=10, m=4)
    opt = oracle.Options()
    opt.max_iter = 30
    res = oracle.solve(pr, opt, capture_iteration=30)
    assert res.iter == 30
    I = Internal(pr)
    x, y, Mx, Mty, _ = I.point(res.primal, res.dual_eq, res.dual_in)
    st = res.state
    assert np.abs(x - st["x"]).max() <= 4e-16 * np.abs(st["x"]).max()
    assert np.array_equal(y, st["y"])
    assert np.abs(Mx - st["Mx"]).max() <= 1e-13 * max(1.0, np.abs(st["Mx"]).max())
    assert np.abs(Mty - st["Mty"]).max() <= 1e-13 * max(1.0, np.abs(st["Mty"]).max())
    s0 = oracle_state0(x, y, Mx, Mty, [1, 2, 2, 2], opt, I.cold_step)
    assert s0["iteration"] == 0 and s0["hist"].shape == (7, 2 * opt.convergence_window) and not s0["hist"].any()
