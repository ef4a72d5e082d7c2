"""CPU-only tests of the device-vector boundary (proxsdp_hip_solve_device, proxsdp_hip_exit_vectors, proxsdp_device_vectors):
the ctypes structure and the Julia shim list the header's members in order, every refusal that is promised "on the host"
happens before a device is touched (this machine may have none: a call that got as far as the device comes back with
PROXSDP_E_HIP), and the expected-value routine the GPU tests compare against (device_result_cases.expected) agrees with the
CPU oracle's formulas and can tell a sum taken in another order."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from oracle import pdhg
from oracle.api import to_standard_form
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd.binding import DeviceVectors

import device_result_cases as D
from kat_problems import sdp_wiki
from test_host_abi import _c_struct_fields

NEW_FUNCTIONS = ("proxsdp_hip_solve_device", "proxsdp_hip_exit_vectors")
E_INVALID, E_HIP, E_UNSUPP = -1, -2, -4


def test_device_vectors_struct_mirrors_the_header_field_by_field():
    header = B.HEADER_PATH.read_text()
    cf = _c_struct_fields(header, "proxsdp_device_vectors")
    assert [f for f, _ in DeviceVectors._fields_] == cf
    assert C.sizeof(DeviceVectors) == 8 + 4 + 4 + 6 * 8 == 64      # no padding
    assert DeviceVectors.primal.offset == 16
    jl = (B.HEADER_PATH.parent.parent / "julia" / "ProxSDPHip.jl").read_text()
    body = re.search(r"struct DeviceVectors\b.*?\n(.*?)\nend", jl, re.S).group(1)
    jf = [re.match(r"\s*(\w+)::", ln).group(1) for ln in body.splitlines() if re.match(r"\s*\w+::", ln)]
    assert jf == cf
    assert ":proxsdp_hip_solve_device" in jl


def test_new_functions_are_exported_and_the_abi_version_stays():
    L = B.lib()
    names = set(B.header_symbols())
    for f in NEW_FUNCTIONS:
        assert f in names, f"{f} is not declared in include/proxsdp_hip.h"
        assert hasattr(L, f), f"{f} is not exported"
    assert L.proxsdp_hip_abi_version() == 10


# ----------------------------------------------------------------- argument errors, straight through the C ABI
FAKE = 0x7F0000001000          # never dereferenced: every call below is refused, or fails, before a kernel could read it


def _ptr(addr):
    return C.cast(C.c_void_p(addr), B.pf64)


def _call(mutate):
    """proxsdp_hip_solve_device on sdp_wiki with well-formed arguments that `mutate` then damages"""
    L = B.lib()
    pr = sdp_wiki(False)
    rng = np.random.default_rng(0)
    M = B._Marshalled(pr)
    o = B.default_options()
    st = dict(primal=rng.standard_normal(pr.n), factors=[(np.array([2.0, 0.5]), rng.standard_normal((3, 2)))])
    S, arr = B._start_struct(pr.n, pr.p, pr.m, B.psd_sides(pr), st)
    sd, od = DeviceVectors(), DeviceVectors()
    for v in (sd, od):
        v.struct_size = C.sizeof(DeviceVectors)
        v.device_id = o.device_id
    sd.dual_eq, sd.dual_in = _ptr(FAKE), _ptr(FAKE + 4096)
    od.primal, od.dual_cone = _ptr(FAKE + 8192), _ptr(FAKE + 12288)
    R = B.Result()
    args = dict(S=S, arr=arr, sd=sd, od=od, M=M, o=o, start=C.byref(S), start_dev=C.byref(sd), out_dev=C.byref(od))
    mutate(args)
    rc = L.proxsdp_hip_solve_device(C.byref(M.P), C.byref(o), C.byref(R), args["start"], args["start_dev"], None,
                                    args["out_dev"])
    return rc, L.proxsdp_hip_last_error().decode()


def _set(which, field, value):
    def m(a):
        setattr(a[which], field, value)
    return m


def _nan_primal(a):
    a["arr"]["primal"][1] = np.nan


def _shard(a):
    cb = B.REDUCE_FN(lambda ctx, ps, ns, pm, nm: 0)
    a["M"].keep.append(cb)
    a["M"].P.reduce_fn = C.cast(cb, C.c_void_p)


INVALID = {
    "start_dev_struct_size": (_set("sd", "struct_size", 56), "struct_size"),
    "out_dev_struct_size": (_set("od", "struct_size", 0), "struct_size"),
    "start_dev_device_id": (_set("sd", "device_id", 3), "device_id"),
    "out_dev_device_id": (_set("od", "device_id", 1), "device_id"),
    "start_dev_dual_cone": (_set("sd", "dual_cone", _ptr(FAKE)), "must be NULL"),
    "start_dev_slack_eq": (_set("sd", "slack_eq", _ptr(FAKE)), "must be NULL"),
    "start_dev_slack_in": (_set("sd", "slack_in", _ptr(FAKE)), "must be NULL"),
    "primal_given_twice": (_set("sd", "primal", _ptr(FAKE)), "both"),
    "solve_from_refusal_struct_size": (_set("S", "struct_size", 8), "proxsdp_start"),
    "solve_from_refusal_nan": (_nan_primal, "non-finite"),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_malformed_device_vectors_are_refused_on_the_host(case):
    mutate, word = INVALID[case]
    rc, msg = _call(mutate)
    assert rc == E_INVALID, (case, rc, msg)
    assert word in msg, (case, msg)


def test_a_shard_is_unsupported():
    rc, msg = _call(_shard)
    assert rc == E_UNSUPP and "shard" in msg, (rc, msg)
    rc, msg = _call(lambda a: (_shard(a), a.update(start=None, start_dev=None)))
    assert rc == E_UNSUPP and "shard" in msg, (rc, msg)


@pytest.mark.skipif(B.device_count() > 0, reason="with a GPU the valid call runs: tests/test_device_results.py")
def test_a_valid_call_reaches_the_device_and_fails_there():
    for mutate in (lambda a: None, lambda a: a.update(start=None, start_dev=None, out_dev=None)):
        rc, msg = _call(mutate)
        assert rc == E_HIP, (rc, msg)


def test_exit_vectors_checks_its_arguments_on_the_host():
    L = B.lib()
    case = D.case_mixed()
    M = B._Marshalled(case.prob, None, 1)
    o = B.default_options()
    nul = C.cast(None, B.pf64)
    x, y = B._f(case.x), B._f(case.y)
    rc = L.proxsdp_hip_exit_vectors(C.byref(M.P), C.byref(o), nul, B._p(y), 0, *([nul] * 8), 0)
    assert rc == E_INVALID and "iterate" in L.proxsdp_hip_last_error().decode()
    _shard(dict(M=M))
    rc = L.proxsdp_hip_exit_vectors(C.byref(M.P), C.byref(o), B._p(x), B._p(y), 0, *([nul] * 8), 0)
    assert rc == E_UNSUPP


def test_python_layer_refuses_what_it_can_see():
    pr = sdp_wiki(False)
    with pytest.raises(ValueError, match="state seam"):
        B.solve(pr, device_out=True, capture_iteration=3)
    with pytest.raises(ValueError, match="state seam|sharded"):
        B.solve(pr, device_out=True, reduce=lambda s, m: None)


# ----------------------------------------------------------------- the expected values against the CPU oracle's formulas
def _oracle_values(case):
    """cache_solution / get_duals / dual_feas of oracle/pdhg.py on the case's iterate (NumPy, its own summation order)"""
    pr = case.prob
    aff, cones = to_standard_form(pr)
    c_orig, var_ordering = pdhg.preprocess(aff, cones)
    a = pdhg.Aux(aff, cones)
    pdhg._setup_blocks(a, cones)
    x, y = np.array(case.x, dtype=float), np.array(case.y, dtype=float)
    pdhg.fix_diag_scaling(x, cones, math.sqrt(2.0))
    c = np.zeros(pr.n) if case.zero_c else c_orig
    dual_eq, dual_in, dual_cone = pdhg.get_duals(y, cones, aff, c, aff.A, aff.G)
    ineq = -min(0.0, float(np.min(dual_in))) if len(dual_in) else 0.0
    one = max([0.0] + [-min(0.0, dual_cone[off]) for (ii, jj, od, off), s in zip(a.tri_idx, cones.sdpcone) if s.sq_side == 1])
    soc = max([0.0] + [-min(0.0, dual_cone[st] - float(np.linalg.norm(dual_cone[st + 1:st + ln]))) for st, ln in a.soc])
    zero = float(np.max(np.abs(dual_cone[a.conelen:]))) if a.conelen < pr.n else 0.0
    neg = [-dual_cone[off:off + s.tri_len] for (ii, jj, od, off), s in zip(a.tri_idx, cones.sdpcone) if s.sq_side >= 2]
    return dict(primal=x[var_ordering], dual_cone=dual_cone[var_ordering], dual_eq=dual_eq, dual_in=dual_in,
                slack_eq=np.asarray(aff.A @ x - aff.b).ravel(), slack_in=np.asarray(aff.G @ x - aff.h).ravel(),
                viol=np.array([ineq, one, soc, zero]), neg=np.concatenate(neg) if neg else np.zeros(0))


SPARSE_CASES = [D.case_one_equality, D.case_one_inequality, D.case_mixed, D.case_grid_tail,
                lambda: D.case_mixed(zero_c=True)]


@pytest.mark.parametrize("make", SPARSE_CASES, ids=["one_equality", "one_inequality", "mixed", "grid_tail", "mixed_zero_c"])
def test_expected_values_restate_the_oracle_formulas(make):
    case = make()
    got, ref = D.expected(case), _oracle_values(case)
    for k in D.KEYS:
        assert got[k].shape == ref[k].shape, k
        assert np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-12), (k, float(np.abs(got[k] - ref[k]).max()))


def test_the_fixtures_name_every_shape_the_issue_asks_for():
    one, two, mixed, grid, dense, zc = D.all_cases()
    assert (one.prob.n, one.prob.p, one.prob.m) == (1, 1, 0) and (two.prob.n, two.prob.p, two.prob.m) == (1, 0, 1)
    pr = mixed.prob
    order = D.solver_layout(mixed)[0]
    assert mixed.index_base == 1 and B.psd_sides(pr) == [3, 1] and [len(s) for s in pr.soc] == [3]
    assert (pr.n, pr.p, pr.m) == (12, 2, 3) and list(order[:3]) != [0, 1, 2]
    M = np.vstack([pr.A.toarray(), pr.G.toarray()])
    assert (np.abs(M).sum(axis=0) == 0).sum() == 1 and (np.abs(M).sum(axis=1) == 0).sum() == 1 and (pr.c == 0).sum() == 1
    pr = grid.prob
    assert pr.n == 257 and pr.p + pr.m == 257 and B.psd_sides(pr) == [22]
    assert pr.A.indptr[41] - pr.A.indptr[40] + pr.G.indptr[41] - pr.G.indptr[40] == 300
    assert int((pr.G.indices == 200 - pr.p).sum()) == 300
    assert dense.prob.M_dense is not None and dense.prob.m > 0 and zc.zero_c and not mixed.zero_c


@pytest.mark.parametrize("make", [D.case_mixed, D.case_grid_tail, lambda: D.case_mixed(zero_c=True)],
                         ids=["mixed", "grid_tail", "mixed_zero_c"])
def test_a_sum_in_reverse_order_changes_a_bit(make):
    """One column's and one row's sum taken backwards must show in the outputs, or an exact comparison with these fixtures
    would not notice a kernel that sums in another order.  (The two one-variable cases and the dense case have no column or
    row with three stored entries, and a sum of two terms from zero is the same both ways: they check other things.)"""
    case = make()
    ref = D.expected(case)
    col = D.expected(case, reverse_col=case.long_col)
    row = D.expected(case, reverse_row=case.long_row)
    assert not D.same_bits(ref["dual_cone"], col["dual_cone"])
    assert not D.same_bits(np.concatenate([ref["slack_eq"], ref["slack_in"]]), np.concatenate([row["slack_eq"], row["slack_in"]]))
    for k in ("primal", "dual_eq", "dual_in"):
        assert D.same_bits(ref[k], col[k]) and D.same_bits(ref[k], row[k])
