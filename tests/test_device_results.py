"""The device exit path and the device-vector entry on the GPU (csrc/exit_device.hip.hpp, proxsdp_hip_solve_device):

* proxsdp_hip_exit_vectors -- the exit kernels through the solver's own launch code -- against the plain-float expected values
  of device_result_cases.py: every vector bit for bit;
* binding.solve(device_out=True) against the host path (proxsdp_hip_solve / _solve_from / _solve_factored) on the same inputs:
  the same solve (scalars, trace, counts) and the same six vectors, bit for bit, on every model class and exit branch;
* chained solves through device tensors against the same chain through host arrays; the finite check that moved to the
  device; the Optimizer layer."""
import numpy as np
import pytest

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

import device_result_cases as D
import kat_problems as K

pytestmark = pytest.mark.gpu

VECTORS = ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in")
SCALARS = ("status", "certificate_found", "primal_feasible_user_tol", "dual_feasible_user_tol", "result_count", "final_rank",
           "iter", "primal_residual", "dual_residual", "objval", "dual_objval", "gap", "dual_feasibility", "status_string")
COUNTS = ("lanczos_matvecs", "lanczos_calls", "lanczos_restarts", "full_eigs", "linesearch_trials", "exit_matvecs",
          "fop_projections", "dense_passes")
TRACE_ELAPSED = 12                                   # wall-clock column: the one two runs do not share


def _opts(**kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def _host(v):
    return v.cpu().numpy() if hasattr(v, "is_cuda") else np.asarray(v)


def _assert_same_result(dev, host, what):
    for k in SCALARS:
        a, b = getattr(dev, k), getattr(host, k)
        assert a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b)), (what, k, a, b)
    for k in COUNTS:
        assert dev.stats[k] == host.stats[k], (what, k, dev.stats[k], host.stats[k])
    keep = [c for c in range(B.TRACE_COLS) if c != TRACE_ELAPSED]
    assert dev.trace.shape == host.trace.shape and np.array_equal(dev.trace[:, keep], host.trace[:, keep]), what
    for k in VECTORS:
        a, b = _host(getattr(dev, k)), getattr(host, k)
        assert a.shape == b.shape and D.same_bits(a, b), (what, k, int((a != b).sum()), float(np.abs(a - b).max(initial=0.0)))


# ----------------------------------------------------------------- the exit kernels against plain-float expected values
@pytest.mark.parametrize("case", D.all_cases(), ids=lambda c: c.name)
def test_exit_vectors_equal_the_expected_values_bit_for_bit(case):
    want = D.expected(case)
    got = B.exit_vectors(case.prob, case.x, case.y, zero_c=case.zero_c, index_base=case.index_base)
    for k in VECTORS + ("neg",):
        assert got[k].shape == want[k].shape, k
        assert D.same_bits(got[k], want[k]), (case.name, k, np.flatnonzero(got[k] != want[k])[:8], got[k][:4], want[k][:4])
    print(case.name, "viol", got["viol"], "expected", want["viol"])
    assert np.array_equal(got["viol"], want["viol"]), (case.name, got["viol"], want["viol"])


# ----------------------------------------------------------------- the same solve, vectors on the device
def _maxcut120():
    return P.maxcut(120, seed=0), dict(max_iter=150), dict(factors=True)


MODELS = {
    "sdp_wiki": lambda: (K.sdp_wiki(False), {}, {}),
    "sdp_plus_soc": lambda: (K.sdp_plus_soc(), {}, {}),
    "soc_norm": lambda: (K.soc_norm(), {}, {}),
    "maxcut120_krylov_factors": _maxcut120,
    "mixed_cones": lambda: (K.mixed_cones(), dict(max_iter=200), {}),
    "sensorloc_long_columns": lambda: (P.sensorloc(20, seed=0), dict(max_iter=300), {}),
    "equilibrated": lambda: (K.sdp_wiki(False), dict(equilibration_force=1), {}),
    "dense_A": lambda: (P.randsdp(5, 4, seed=2, dense=True), dict(max_iter=300), {}),
    "infeasible_certificate": lambda: (K.infeasible_lp(), dict(max_iter=2000, max_obj=10.0, certificate_search=1), {}),
    "unbounded_certificate": lambda: (K.unbounded_lp(), dict(max_obj=1e300, certificate_search=1), {}),
    "index_base_1": lambda: (K.sdp_plus_soc(), {}, dict(index_base=1)),
    "mixed_fixture_index_base_1": lambda: (D.case_mixed().prob, dict(max_iter=200), dict(index_base=1)),
}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_solve_device_is_the_host_solve_bit_for_bit(name):
    import torch
    pr, okw, skw = MODELS[name]()
    host = B.solve(pr, _opts(**okw), trace_capacity=400, **skw)
    dev = B.solve(pr, _opts(**okw), trace_capacity=400, device_out=True, **skw)
    print(name, "status", host.status, "iter", host.iter, "dual_feasibility", host.dual_feasibility, "exit_time host",
          host.stats["exit_time"], "device", dev.stats["exit_time"])
    assert all(isinstance(getattr(dev, k), torch.Tensor) and getattr(dev, k).is_cuda for k in VECTORS)
    _assert_same_result(dev, host, name)
    if name.endswith("certificate"):
        assert host.certificate_found, "the case no longer reaches the certificate exit"
    if skw.get("factors"):
        assert host.stats["exit_matvecs"] > 0, "the lambda_min run did not take the Krylov branch"
        for (v1, V1, i1), (v2, V2, i2) in zip(dev.psd_factors, host.psd_factors):
            assert np.array_equal(v1, v2) and np.array_equal(V1, V2) and i1 == i2


def test_host_arrays_and_device_buffers_in_one_call_receive_the_same_values():
    """proxsdp_hip_solve_device straight through ctypes: res arrays and out_dev buffers both given, primal not wanted on the
    device, a NULL member left alone"""
    import ctypes as C
    import torch
    pr = K.sdp_plus_soc()
    ref = B.solve(pr, _opts())
    M = B._Marshalled(pr)
    n, p, m = pr.n, pr.p, pr.m
    lens = dict(primal=n, dual_cone=n, dual_eq=p, dual_in=m, slack_eq=p, slack_in=m)
    host = {k: np.full(max(v, 1), np.nan) for k, v in lens.items()}
    tens = {k: torch.full((v,), float("nan"), dtype=torch.float64, device="cuda:0") for k, v in lens.items() if k != "primal"}
    R = B.Result()
    for k in lens:
        setattr(R, k, B._p(host[k]))
    out = B._device_vectors(0, **{k: (t, lens[k]) for k, t in tens.items()})
    o = _opts()
    torch.cuda.synchronize()
    B._check(B.lib().proxsdp_hip_solve_device(C.byref(M.P), C.byref(o), C.byref(R), None, None, None, C.byref(out)))
    for k, v in lens.items():
        assert D.same_bits(host[k][:v], getattr(ref, k)), k
        if k in tens:
            assert D.same_bits(tens[k].cpu().numpy(), getattr(ref, k)), k


# ----------------------------------------------------------------- chains
@pytest.fixture(scope="module")
def chain():
    """Max-Cut n = 120 solved cold with factors, then a perturbed instance (edge weights moved by up to 1 %) from that result:
    once through host arrays, once through device tensors"""
    p1 = P.maxcut(120, seed=0)
    rng = np.random.default_rng(7)
    p2 = P.maxcut(120, seed=0)
    p2.c = p2.c * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, p2.n))
    h1 = B.solve(p1, _opts(), factors=True, trace_capacity=4000)
    h2 = B.solve(p2, _opts(), start=h1, trace_capacity=4000)
    d1 = B.solve(p1, _opts(), factors=True, trace_capacity=4000, device_out=True)
    d2 = B.solve(p2, _opts(), start=d1, trace_capacity=4000, device_out=True)
    return h1, h2, d1, d2


def test_chain_through_device_tensors_is_the_chain_through_host_arrays(chain):
    h1, h2, d1, d2 = chain
    print("cold %d iterations, warm re-solve of the perturbed instance %d" % (h1.iter, h2.iter))
    assert d1.primal.is_cuda and d2.primal.is_cuda
    assert h1.status == 1 and h2.status == 1 and h2.iter < h1.iter
    _assert_same_result(d1, h1, "cold")
    _assert_same_result(d2, h2, "warm")


def test_device_start_from_tensors_without_factors(chain):
    """primal and duals as CUDA tensors in a start dictionary, beside a host-side target rank: the gather reads them where
    they are; dual_eq alone on the device and dual_in on the host mix"""
    h1, _, d1, _ = chain
    pr = P.maxcut(120, seed=0)
    rank = h1.psd_factors[0][2]["rank_found"]
    o = dict(max_iter=60)
    ref = B.solve(pr, _opts(**o), start=dict(primal=h1.primal, dual_eq=h1.dual_eq, dual_in=h1.dual_in, target_rank=[rank + 1]),
                  trace_capacity=100)
    dev = B.solve(pr, _opts(**o), start=dict(primal=d1.primal, dual_eq=d1.dual_eq, dual_in=d1.dual_in, target_rank=[rank + 1]),
                  trace_capacity=100)
    _assert_same_result(dev, ref, "device start, host result")
    mix = B.solve(pr, _opts(**o), start=dict(primal=h1.primal, dual_eq=d1.dual_eq, dual_in=h1.dual_in, target_rank=[rank + 1]),
                  trace_capacity=100, device_out=True)
    _assert_same_result(mix, ref, "mixed start, device result")


@pytest.mark.parametrize("vector", ["primal", "dual_eq"])
def test_a_non_finite_device_start_is_refused_before_the_first_iteration(chain, vector):
    _, _, d1, _ = chain
    pr = P.maxcut(120, seed=0)
    st = dict(primal=d1.primal.clone(), dual_eq=d1.dual_eq.clone())
    st[vector][3] = float("nan")
    with pytest.raises(B.ProxSDPHipError) as e:
        B.solve(pr, _opts(), start=st, device_out=True)
    assert e.value.code == -1 and vector in str(e.value), str(e.value)             # PROXSDP_E_INVALID, and the vector's name


def test_optimizer_passes_device_out_through():
    import torch
    pr = K.sdp_wiki(True)
    oh, od = Optimizer(), Optimizer()
    sh, sd = oh.optimize(pr), od.optimize(pr, device_out=True)
    assert isinstance(od.variable_primal(), torch.Tensor) and od.variable_primal().is_cuda
    assert od.objective_value() == oh.objective_value() and od.termination_status() == oh.termination_status()
    assert sd.status == sh.status and sd.iter == sh.iter
    assert D.same_bits(od.constraint_primal_psd(0).cpu().numpy(), oh.constraint_primal_psd(0))
    assert D.same_bits(od.constraint_dual_zeros().cpu().numpy(), oh.constraint_dual_zeros())
