"""equilibration / equilibration_force and approx_norm = false on the dense-A entry (proxsdp_problem.M_dense): the set-up
runs on the device -- one pass over the borrowed matrix for the row sums and the extrema, the scaling carried in the
vectors of the dense products, sigma_max by Lanczos through those products -- and is checked against the oracle, NumPy and
the library's own CSC path fed the same numbers (which has served these options from the host all along)."""
import numpy as np
import pytest

import oracle
from oracle import Options
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

from dense_scaling_cases import as_sparse, full_matrix, inst_a, inst_b, inst_c, offdiag_scale, oracle_scaling

pytestmark = pytest.mark.gpu

CASES = {"A": inst_a, "B": inst_b, "C": inst_c}
# the five option sets of test_equilibration_and_spectral_norm_against_oracle
KWS = [dict(equilibration_force=1, equilibration_reference_aliasing=0), dict(approx_norm=0),
       dict(equilibration_force=1, approx_norm=0, equilibration_reference_aliasing=0),
       dict(equilibration_force=1), dict(equilibration_force=1, approx_norm=0)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert B.device_count() > 0, "no HIP device: the product path has no CPU fallback"


def _opts(**kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def _trace_cols(ref_trace):
    return np.array([[t["prim_obj"], t["dual_obj"], t["gap"], t["feas"], t["primal_step"], t["trials"]] for t in ref_trace])


def _oracle(pr, **kw):
    o = Options()
    for k, v in kw.items():
        o.set(k, v if k in ("max_iter",) else bool(v))
    return oracle.solve(as_sparse(pr), o, trace=True)


def _on_device(pr):
    import torch
    return P.Problem(n=pr.n, A=pr.A, b=pr.b, G=pr.G, h=pr.h, c=pr.c, psd=pr.psd, name=pr.name,
                     M_dense=torch.from_numpy(np.asarray(pr.M_dense)).to("cuda:0"))


# ----------------------------------------------------------------- set-up
@pytest.mark.parametrize("name,aliasing", [("A", 0), ("B", 0), ("C", 0), ("B", 1), ("C", 1)])
def test_dense_scaling_entry_against_oracle_and_numpy(name, aliasing):
    """E, D against oracle.pdhg.equilibrate (1e-9: summation order), ||E M D S||_F against NumPy (1e-12), sigma_max against
    numpy.linalg.svd (1e-10: where SciPy's svds and the library's host Lanczos already differ); a host pointer and a
    device pointer give the same bits.  (A with the aliasing is the chaotic case: see the host test.)"""
    pr = CASES[name]()
    M, s = full_matrix(pr), offdiag_scale(pr)
    Eo, Do = oracle_scaling(pr, aliasing)
    o = _opts(equilibration_force=1, approx_norm=0, equilibration_reference_aliasing=aliasing)
    E, D, fro, sig, eq = B.dense_scaling(pr, o)
    assert eq
    eE, eD = np.max(np.abs(E - Eo) / Eo), np.max(np.abs(D - Do) / Do)
    Ms = E[:, None] * M * (D * s)[None, :]
    eF = abs(fro - np.linalg.norm(Ms)) / np.linalg.norm(Ms)
    sv = np.linalg.svd(Ms, compute_uv=False)[0]
    eS = abs(sig - sv) / sv
    print(f"{name} aliasing={aliasing}: rel err E {eE:.2e} D {eD:.2e} frob {eF:.2e} sigma_max {eS:.2e}")
    assert eE <= 1e-9 and eD <= 1e-9
    assert eF <= 1e-12
    assert eS <= 1e-10
    E2, D2, fro2, sig2, eq2 = B.dense_scaling(_on_device(pr), o)
    assert eq2 and np.array_equal(E, E2) and np.array_equal(D, D2) and fro == fro2 and sig == sig2
    # sigma_max is computed only on request
    assert B.dense_scaling(pr, _opts(equilibration_force=1, equilibration_reference_aliasing=aliasing))[3] == 0.0


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_dense_sigma_max_without_equilibration(name):
    pr = CASES[name]()
    Ms = full_matrix(pr) * offdiag_scale(pr)[None, :]
    E, D, fro, sig, eq = B.dense_scaling(pr, _opts(approx_norm=0))
    assert not eq and np.all(E == 1.0) and np.all(D == 1.0)
    sv = np.linalg.svd(Ms, compute_uv=False)[0]
    print(f"{name}: frob {abs(fro - np.linalg.norm(Ms)) / np.linalg.norm(Ms):.2e} sigma_max {abs(sig - sv) / sv:.2e}")
    assert abs(fro - np.linalg.norm(Ms)) <= 1e-12 * np.linalg.norm(Ms)
    assert abs(sig - sv) <= 1e-10 * sv


def test_plain_equilibration_switches_itself_off_unless_nearly_constant():
    """pdhg.jl:66-73: `equilibration` survives only if min(M)/max(M) > equilibration_limit, implicit zeros of G counted."""
    o = _opts(equilibration=1, equilibration_reference_aliasing=0)
    assert B.dense_scaling(inst_c(), o)[4]
    for pr in (inst_c(dent=True), inst_a()):
        E, D, fro, sig, eq = B.dense_scaling(pr, o)
        assert not eq and np.all(E == 1.0) and np.all(D == 1.0)


# ----------------------------------------------------------------- solves
@pytest.mark.parametrize("kw", KWS)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_dense_solve_with_scaling_against_oracle_and_csc_path(name, kw):
    pr = CASES[name]()
    iters = 300
    s_d = Optimizer(max_iter=iters, **kw).optimize(pr, trace_capacity=iters)
    T = s_d.trace[:, [1, 2, 3, 4, 7, 11]]
    assert s_d.stats["dense_setup_passes"] == (1 if "equilibration_force" in kw else 0)
    assert (s_d.stats["dense_sigma_steps"] > 0) == ("approx_norm" in kw)
    if name == "A" and kw.get("equilibration_force") and kw.get("equilibration_reference_aliasing", 1):
        # The reference's aliased scaling iteration with bound rows present is chaotic: on the oracle alone a 1e-15 relative
        # perturbation of the data moves E by 12 % after its 1000 iterations, so two correct restatements produce different
        # -- equally valid -- scalings and different iterates.  What no diagonal scaling can change is asserted: the run
        # is finite, and the returned slack is A x of the returned primal with the caller's unscaled A.
        assert np.all(np.isfinite(s_d.trace[:, 1:8]))
        ax = np.asarray(pr.M_dense) @ s_d.primal
        sc = max(1.0, np.abs(ax).max())
        print(f"A aliased {kw}: max |slack_eq + b - A x| / scale = {np.abs(s_d.slack_eq + pr.b - ax).max() / sc:.2e}")
        assert np.abs(s_d.slack_eq + pr.b - ax).max() <= 1e-9 * sc
        return
    s_s = Optimizer(max_iter=iters, **kw).optimize(as_sparse(pr), trace_capacity=iters)
    ref = _oracle(pr, max_iter=iters, **kw)
    G = _trace_cols(ref.trace)
    S = s_s.trace[:, [1, 2, 3, 4, 7, 11]]
    for what, other, st, it in (("oracle", G, ref.status, ref.iter), ("csc", S, s_s.status, s_s.iter)):
        m = min(len(other), len(T), 40)
        sc = max(1.0, np.abs(other[:m]).max())
        err = np.abs(T[:m] - other[:m]) / (1e-9 * sc + 1e-6 * np.abs(other[:m]))
        print(f"{name} {kw} vs {what}: status {s_d.status}/{st} iter {s_d.iter}/{it} first-{m} trace err / bound {err.max():.3g}")
        assert s_d.status == st and s_d.iter == it
        assert np.array_equal(T[:, 5], other[:, 5]), "linesearch trials"
        assert np.allclose(T[:m], other[:m], rtol=1e-6, atol=1e-9 * sc)


def test_plain_equilibration_engages_on_the_nearly_constant_model():
    """The switch: on C plain `equilibration = true` stays on and the solve reaches OPTIMAL in far fewer iterations (the
    oracle's count, to 2 %) than without; with one entry set to 0.5 it switches itself off and the solve is the plain one,
    bit for bit."""
    kw = dict(equilibration=1, equilibration_reference_aliasing=0)
    pr = inst_c()
    ref_eq = _oracle(pr, **kw)
    ref_plain = _oracle(pr)
    assert ref_eq.status == 1 and ref_plain.status == 1
    sol = Optimizer(**kw).optimize(pr)
    print(f"C: iterations library {sol.iter}, oracle equilibrated {ref_eq.iter}, oracle plain {ref_plain.iter}")
    assert sol.status == 1 and sol.stats["dense_setup_passes"] == 1
    assert abs(sol.iter - ref_eq.iter) <= 0.02 * ref_eq.iter
    assert abs(sol.iter - ref_plain.iter) > 0.1 * ref_plain.iter
    assert abs(sol.objval - ref_eq.objval) <= 1e-3 * (1 + abs(ref_eq.objval))        # (10 x the default tol_gap)
    prd = inst_c(dent=True)
    a = Optimizer(max_iter=300, **kw).optimize(prd, trace_capacity=300)
    b = Optimizer(max_iter=300).optimize(prd, trace_capacity=300)
    assert a.iter == b.iter and np.array_equal(a.trace[:, 1:12], b.trace[:, 1:12])
    assert np.array_equal(a.primal, b.primal) and np.array_equal(a.dual_eq, b.dual_eq)


def test_borrowed_device_matrix_is_untouched_by_the_scaled_solve():
    import torch
    pr = _on_device(inst_a())
    M0 = pr.M_dense.clone()
    sol = Optimizer(max_iter=50, equilibration_force=1, approx_norm=0).optimize(pr, trace_capacity=50)
    assert sol.iter == 50 and sol.stats["dense_setup_passes"] == 1 and sol.stats["dense_sigma_steps"] > 0
    assert torch.equal(pr.M_dense, M0)


def test_scaled_solve_at_the_full_size():
    """BASELINE config 3 at its actual size (4000 x 2 001 000 doubles = 64 GB in HBM, borrowed): forced equilibration and
    the device sigma_max.  sigma_max against a 60-step power iteration in torch on the same tensor, the scalings applied
    to the vectors and G on the host."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 90 * 2 ** 30:
        pytest.skip("needs 90 GB of free HBM")
    n, m = 2000, 4000
    pr = P.randsdp_device(n, m, seed=0, device="cuda:0")
    M = pr.M_dense
    kw = dict(approx_norm=0, equilibration_force=1, equilibration_reference_aliasing=0)
    E, D, fro, sig, eq = B.dense_scaling(pr, _opts(**kw))
    assert eq and np.all(np.isfinite(E)) and np.all(np.isfinite(D)) and sig > 0 and sig <= fro
    ds = D * offdiag_scale(pr)
    Ea_t = torch.from_numpy(E[:m]).to("cuda:0")
    G, Eg = pr.G.tocsr(), E[m:]
    v = np.full(pr.n, 1.0 / np.sqrt(pr.n))
    lam = 0.0
    for _ in range(60):                                        # power iteration on (E M D S)'(E M D S)
        dv = ds * v
        ua = Ea_t * (M @ torch.from_numpy(dv).to("cuda:0"))
        ug = Eg * (G @ dv)
        w = ds * ((M.T @ (Ea_t * ua)).cpu().numpy() + G.T @ (Eg * ug))
        lam = float(v @ w)
        v = w / np.linalg.norm(w)
    print(f"full size: sigma_max entry {sig:.12e}, power iteration {np.sqrt(lam):.12e}, rel {abs(sig - np.sqrt(lam)) / sig:.2e}")
    assert abs(sig - np.sqrt(lam)) <= 1e-6 * sig
    del ua, Ea_t
    iters = 12
    sol = Optimizer(max_iter=iters, initial_target_rank=50, max_target_rank_krylov_eigs=50, **kw).optimize(pr, trace_capacity=iters)
    assert sol.iter == iters and sol.stats["dense_setup_passes"] == 1 and sol.stats["dense_sigma_steps"] > 0
    assert np.all(np.isfinite(sol.trace[:, 1:8]))
    del M
    torch.cuda.empty_cache()
