"""The certified dual bound without a device (proxsdp_host_dual_bound, proxsdp_host_cholesky; include/proxsdp_hip.h "a
certified dual bound"): the host half of csrc/dual_bound_host.hpp through the library.  Fixtures and the NumPy side of the
checks: tests/bound_cases.py.  The device route is tests/test_dual_bound.py."""
import ctypes as C
import dataclasses
import pathlib

import numpy as np
import pytest
import scipy.sparse as sp

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P

import bound_cases as K

E_INVALID, E_UNSUPP = -1, -4
NONE = np.zeros(0)
HOST_SIDES = (1, 2, 5, 16, 17, 33, 65)


def test_entries_are_declared_and_exported_and_the_abi_version_stays():
    L = B.lib()
    names = set(B.header_symbols())
    for sym in ("proxsdp_hip_model_bound", "proxsdp_host_dual_bound", "proxsdp_hip_cholesky", "proxsdp_host_cholesky"):
        assert sym in names and hasattr(L, sym), sym
    assert L.proxsdp_hip_abi_version() == 10


def test_struct_size_follows_the_field_list():
    # int64, 2 x int32 | 3 + 7 pointers | 2 doubles, int64, 2 doubles
    assert C.sizeof(B.DualBoundIO) == 8 + 2 * 4 + 10 * 8 + 2 * 8 + 8 + 2 * 8


@pytest.mark.parametrize("side", K.FACTOR_SIDES)
def test_the_serial_cholesky_on_the_factorisation_cases(side):
    for kind in ("unit", "scaled"):
        L = K.integer_factor(side, 0, kind)
        fail, R = B.host_cholesky(K.product(L))
        assert fail == -1 and np.array_equal(R, L.T), (side, kind)
    A, eps = K.minus_eps(K.product(K.integer_factor(side, 0, "unit")))
    fail = B.host_cholesky(A, want_factor=False)[0]
    if side <= 2:
        assert fail == -1
    else:
        assert K.indefinite_witness(K.product(K.integer_factor(side, 0, "unit"))) and 0 <= fail < side, (side, fail)
    A, L = K.last_pivot_bad(side, 1)
    fail, R = B.host_cholesky(A)
    assert fail == side - 1 and np.array_equal(R[:side - 1, :], L.T[:side - 1, :])
    assert B.host_cholesky(np.zeros((side, side)), want_factor=False)[0] == 0
    assert B.host_cholesky(np.full((side, side), np.nan), want_factor=False)[0] == 0
    A = K.spd_real(side, 0)
    fail, R = B.host_cholesky(A)
    assert fail == -1
    K.assert_backward_error(A, R, f"side {side}")


@pytest.mark.parametrize("side", HOST_SIDES)
def test_the_bound_never_exceeds_the_known_optimum_and_is_tight(side):
    case = K.known_optimum(side)
    pr, p_star = case["problem"], case["p_star"]
    for kind in ("exact", "uniform", "seeded"):
        ye, Zt, lam = K.duals(case, kind)
        db = B.host_dual_bound(pr, ye, NONE)
        what = f"side {side}, {kind} duals"
        assert db.certified.all() and db.bound <= p_star, (what, db.bound, p_star)          # an exact comparison
        assert db.dual_objective == -float(ye.sum()) and db.bytes_allocated == 0, what
        if side == 1:
            assert db.factorisations[0] == 0 and db.shift[0] == 0.0
            assert db.lambda_lower[0] <= Zt[0, 0] and db.lambda_lower[0] >= Zt[0, 0] - 1e-12 * (1 + abs(Zt[0, 0]))
            continue
        assert 1 <= db.factorisations[0] <= 19
        K.assert_tight(db, 0, Zt, what)
        ideal = -float(ye.sum()) + side * min(0.0, float(np.linalg.eigvalsh(Zt).min()))
        assert db.bound >= ideal - 1.01 * db.loss - 1e-9 * (1.0 + np.abs(ye).sum()), (what, db.bound, ideal, db.loss)


def test_trace_caps_derived_given_refused_and_blind_to_inequality_rows():
    case = K.known_optimum(9)
    pr, y = case["problem"], case["y"].astype(float)
    derived = B.host_dual_bound(pr, y - 0.25, NONE)
    up1 = np.nextafter(1.0, np.inf)
    T = 0.0
    for _ in range(9):
        T = np.nextafter(T + up1, np.inf)
    assert derived.trace[0] == T
    given = B.host_dual_bound(pr, y - 0.25, NONE, trace_cap=[T])
    assert given.bound == derived.bound and given.lambda_lower[0] == derived.lambda_lower[0]
    assert B.host_dual_bound(pr, y - 0.25, NONE, trace_cap=[2 * T]).bound < derived.bound
    # rows a X_ii = b with another a and b: the cap is b / a rounded up; a second row on the same diagonal: the smaller cap
    A2 = sp.csc_matrix(pr.A * 4.0)
    scaled = dataclasses.replace(pr, A=A2, b=np.full(9, 12.0))
    assert B.host_dual_bound(scaled, y / 4.0, NONE).trace[0] == pytest.approx(27.0, rel=1e-14)
    extra = sp.vstack([pr.A, sp.csc_matrix(([2.0], ([0], [0])), shape=(1, pr.n))], format="csc")
    two = dataclasses.replace(pr, A=extra, b=np.concatenate([pr.b, [1.0]]))
    assert B.host_dual_bound(two, np.concatenate([y, [0.0]]), NONE).trace[0] == pytest.approx(8.5, rel=1e-14)
    # an uncovered diagonal, a negative quotient, a row with two entries: refused, the cone named
    for bad in (dataclasses.replace(pr, A=sp.csc_matrix(pr.A[:-1, :]), b=pr.b[:-1]),
                dataclasses.replace(pr, b=np.concatenate([pr.b[:-1], [-1.0]])),
                dataclasses.replace(pr, A=sp.csc_matrix(pr.A + sp.csc_matrix(([1.0], ([8], [1])), shape=pr.A.shape)))):
        with pytest.raises(B.ProxSDPHipError) as e:
            B.host_dual_bound(bad, np.zeros(bad.A.shape[0]), NONE)
        assert e.value.code == E_INVALID and "cone 0" in str(e.value)
        assert B.host_dual_bound(bad, np.zeros(bad.A.shape[0]), NONE, trace_cap=[9.0]).certified.all()
    # inequality rows -- the rows a change_rows adds -- do not enter the caps, even on a diagonal variable
    G = sp.csc_matrix(([1.0, 1.0], ([0, 1], [0, 2])), shape=(2, pr.n))
    rows = dataclasses.replace(pr, G=G, h=np.array([0.5, 3.0]))
    assert B.host_dual_bound(rows, y, np.zeros(2)).trace[0] == T


def test_rows_changed_through_the_rows_plan_are_the_ones_the_caps_and_the_bound_see():
    """the problem a change_rows leaves behind, as proxsdp_host_model_rows_plan stacks it (kept rows, then the new ones):
    the bound of that problem is the bound of the stacked problem built by hand, and its caps are the equality rows'"""
    pr, best = K.maxcut16_with_triangles(rows=12)
    base = dataclasses.replace(pr, G=sp.csc_matrix(pr.G[:4, :]), h=pr.h[:4])
    Gn = sp.csr_matrix(pr.G[4:, :])
    plan = B.host_model_rows_plan(base, add=((Gn.indptr, Gn.indices, Gn.data), pr.h[4:]), drop=[1])
    assert plan["m"] == 11 and plan["kept"].tolist() == [0, 2, 3] + [-1] * 8
    kept = plan["kept"][plan["kept"] >= 0]
    stacked = dataclasses.replace(pr, G=sp.vstack([pr.G[kept, :], pr.G[4:, :]], format="csc"),
                                  h=np.concatenate([pr.h[kept], pr.h[4:]]))
    assert np.array_equal(plan["bh"], np.concatenate([stacked.b, stacked.h]))        # the planner's [b; h'] is the stacked one
    rng = np.random.default_rng(3)
    ye, yi = -rng.uniform(1.0, 3.0, 16), rng.uniform(-0.5, 0.5, 11)
    db = B.host_dual_bound(stacked, ye, yi)
    assert db.trace[0] == B.host_dual_bound(base, ye, np.zeros(4)).trace[0]
    assert -db.bound >= best


def test_negative_inequality_duals_are_clamped_and_the_bound_stays_above_the_largest_cut():
    pr, best = K.maxcut16_with_triangles()
    Cm = K.dual_matrices(pr, np.zeros(16), np.zeros(pr.G.shape[0]))[0]
    rng = np.random.default_rng(11)
    for trial in range(4):
        yi = rng.uniform(-0.4, 0.4, pr.G.shape[0])
        assert (yi > 0).any() and (yi < 0).any()
        # a diagonally dominant start, then pushed off it: any y gives a bound
        ye = -np.diag(Cm) + np.abs(Cm - np.diag(np.diag(Cm))).sum(axis=1) * (1.0 - 0.3 * trial) + rng.uniform(-0.2, 0.2, 16)
        db = B.host_dual_bound(pr, ye, yi)
        clamped = B.host_dual_bound(pr, ye, np.maximum(yi, 0.0))
        assert db.bound == clamped.bound and db.lambda_lower[0] == clamped.lambda_lower[0], trial
        upper = pr.user_objective(db.bound)
        print(f"trial {trial}: upper bound {upper:.6f}, largest cut {best}, shift {db.shift[0]:.4g}")
        assert db.certified.all() and upper >= best, (trial, upper, best)
        K.assert_tight(db, 0, K.dual_matrices(pr, ye, yi)[0], f"maxcut 16, trial {trial}")
        # the unclamped duals would give another (invalid) figure: the clamp is not a no-op on this instance
        assert db.dual_objective == pytest.approx(-(pr.b @ ye) - pr.h @ np.maximum(yi, 0.0), rel=1e-13)


def test_a_hopeless_matrix_is_not_certified_and_the_call_still_returns():
    """nu is rounded UP, so sigma_12 = nu >= ||Z~||_inf always leaves a matrix with positive pivots in exact arithmetic: a
    matrix of ordinary scale is certified (Z = -I: sigma* a little above 1).  What is hopeless is a scale at which nu itself
    overflows: all entries -8e307 (finite, NaN-free) have the row sum +inf; the cone is then not certified, no factorisation
    is tried, the bound is -inf and the call still returns 0."""
    s = 6
    N = P.sympackedlen(s)
    pr = P.Problem(n=N, A=P._empty(N), b=NONE, G=P._empty(N), h=NONE, c=K.tri_vector(-np.eye(s)),
                   psd=[np.arange(N, dtype=np.int64)])
    ok = B.host_dual_bound(pr, NONE, NONE, trace_cap=[float(s)])
    assert ok.certified[0] and 1.0 <= ok.shift[0] <= 1.0 + 1e-12 and -s * (1 + 1e-9) <= ok.bound <= -s
    db = B.host_dual_bound(dataclasses.replace(pr, c=K.tri_vector(np.full((s, s), -8e307))), NONE, NONE, trace_cap=[float(s)])
    assert not db.certified[0] and db.factorisations[0] == 0
    assert db.bound == -np.inf and db.lambda_lower[0] == -np.inf and db.shift[0] == np.inf


def test_two_cones_add_up():
    a, b = K.known_optimum(5), K.known_optimum(7, seed=1)
    pr = P.block_diag_problems([a["problem"], b["problem"]])
    ya, _, _ = K.duals(a, "uniform")
    yb, _, _ = K.duals(b, "seeded")
    db = B.host_dual_bound(pr, np.concatenate([ya, yb]), NONE)
    one = [B.host_dual_bound(a["problem"], ya, NONE), B.host_dual_bound(b["problem"], yb, NONE)]
    assert db.certified.all() and db.bound <= a["p_star"] + b["p_star"]
    for k in range(2):
        for name in ("shift", "lambda_lower", "radius", "delta", "trace", "factorisations"):
            assert getattr(db, name)[k] == getattr(one[k], name)[0], (k, name)
    assert db.bound == pytest.approx(one[0].bound + one[1].bound, rel=1e-13)


def _raw(pr, ye, yi, **over):
    """a direct call of proxsdp_host_dual_bound with every argument open to a fault; returns (code, message, arrays)"""
    L = B.lib()
    M = sp.vstack([sp.csc_matrix(pr.A), sp.csc_matrix(pr.G)], format="csc")
    M.sort_indices()
    cp, rv, nz = B._i(M.indptr), B._i(M.indices), B._f(M.data)
    Mc = B.CSC(M.shape[0], pr.n, B._p(cp, B.pi64), B._p(rv, B.pi64), B._p(nz))
    ptr = B._i(np.cumsum([0] + [len(v) for v in pr.psd]))
    idx = B._i(np.concatenate(pr.psd))
    bh, c = B._f(np.concatenate([pr.b, pr.h])), B._f(pr.c)
    Q, arr = B._bound_struct(len(pr.psd), over.pop("trace_cap", None), sentinel=7)
    ye, yi = B._f(ye), B._f(yi)
    Q.dual_eq, Q.dual_in = B._p(ye if len(ye) else np.zeros(1)), B._p(yi if len(yi) else np.zeros(1))
    args = dict(n=pr.n, p=pr.A.shape[0], m=pr.G.shape[0], c=B._p(c), M=C.byref(Mc), bh=B._p(bh if len(bh) else np.zeros(1)),
                n_psd=len(pr.psd), ptr=B._p(ptr, B.pi64), idx=B._p(idx, B.pi64), base=0, q=C.byref(Q))
    for k, v in list(over.items()):
        if k.startswith("Q_"):
            setattr(Q, k[2:], v); over.pop(k)
    args.update(over)
    rc = L.proxsdp_host_dual_bound(args["n"], args["p"], args["m"], args["c"], args["M"], args["bh"], args["n_psd"],
                                   args["ptr"], args["idx"], args["base"], args["q"])
    return rc, L.proxsdp_hip_last_error().decode(), arr


def _untouched(arr):
    return all(np.all(a == 7) for k, a in arr.items() if k != "trace_cap")


def test_refusals_need_no_device_and_write_nothing():
    case = K.known_optimum(5)
    pr, y = case["problem"], case["y"].astype(float)
    rc, _, arr = _raw(pr, y, NONE)
    assert rc == 0 and not _untouched(arr)
    null = C.POINTER(C.c_double)()
    for over, word in ((dict(q=None), "NULL"), (dict(Q_struct_size=8), "struct_size"), (dict(Q_on_device=2), "on_device"),
                       (dict(Q_on_device=1), "on_device"), (dict(Q_dual_eq=null), "dual_eq"), (dict(Q_shift=null), "output"),
                       (dict(Q_certified=C.POINTER(C.c_int32)()), "output"), (dict(trace_cap=[-1.0]), "trace_cap"),
                       (dict(trace_cap=[np.inf]), "trace_cap"), (dict(trace_cap=[np.nan]), "trace_cap"),
                       (dict(base=2), "index_base"), (dict(c=None), "NULL"), (dict(M=None), "NULL"), (dict(n=0), "n"),
                       (dict(n_psd=0), "n_psd"), (dict(p=4), "shape")):
        rc, msg, arr = _raw(pr, y, NONE, **over)
        assert rc == E_INVALID and word in msg and _untouched(arr), (over, rc, msg)
    for bad in (np.nan, np.inf, -np.inf):
        yy = y.copy(); yy[2] = bad
        rc, msg, arr = _raw(pr, yy, NONE)
        assert rc == E_INVALID and "dual_eq" in msg and _untouched(arr)
    G = sp.csc_matrix(([1.0], ([0], [1])), shape=(1, pr.n))
    rc, msg, arr = _raw(dataclasses.replace(pr, G=G, h=np.ones(1)), y, np.array([np.nan]))
    assert rc == E_INVALID and "dual_in" in msg and _untouched(arr)
    rc, msg, arr = _raw(dataclasses.replace(pr, c=np.where(np.arange(pr.n) == 3, np.inf, pr.c)), y, NONE)
    assert rc == E_INVALID and "c" in msg and _untouched(arr)
    # a variable outside every cone: not served; a cone list that is no triangle or repeats a variable: malformed
    free = dataclasses.replace(pr, psd=[pr.psd[0][:10]])
    rc, msg, arr = _raw(free, y, NONE)
    assert rc == E_UNSUPP and "outside every cone" in msg and _untouched(arr)
    rc, msg, arr = _raw(dataclasses.replace(pr, psd=[pr.psd[0][:9]]), y, NONE)
    assert rc == E_INVALID and "triangle" in msg and _untouched(arr)
    twice = pr.psd[0].copy(); twice[4] = twice[3]
    rc, msg, arr = _raw(dataclasses.replace(pr, psd=[twice]), y, NONE)
    assert rc == E_INVALID and "twice" in msg and _untouched(arr)
    L = B.lib()
    fail = C.c_int64(7)
    assert L.proxsdp_host_cholesky(None, 1, 0.0, None, C.byref(fail)) == E_INVALID
    assert L.proxsdp_host_cholesky(B._p(np.ones(1)), 46341, 0.0, None, C.byref(fail)) == E_INVALID
    assert L.proxsdp_host_cholesky(B._p(np.ones(1)), 1, -0.5, None, C.byref(fail)) == E_INVALID and fail.value == 7
    # the handle entry decides its struct checks before it looks at a handle
    Q, arr = B._bound_struct(1, sentinel=7)
    assert L.proxsdp_hip_model_bound(None, C.byref(Q)) == E_INVALID and "handle" in L.proxsdp_hip_last_error().decode()
    Q.struct_size = 16
    assert L.proxsdp_hip_model_bound(None, C.byref(Q)) == E_INVALID and "struct_size" in L.proxsdp_hip_last_error().decode()
    assert L.proxsdp_hip_model_bound(None, None) == E_INVALID and _untouched(arr)


def test_stand_alone_check_of_the_host_half_under_the_sanitizers(tmp_path):
    """tests/c_harness/dual_bound_check.cpp: dual_bound_host.hpp alone, no HIP, no library.  Built with the address and
    undefined-behaviour sanitizers, their runtimes linked INTO the program, and run directly; nothing loaded into Python runs
    under a sanitizer."""
    import subprocess
    root = pathlib.Path(__file__).resolve().parent.parent
    exe = tmp_path / "dual_bound_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall", "-Werror", f"-I{root / 'proxsdp.jl_amd' / 'csrc'}",
           str(root / "tests" / "c_harness" / "dual_bound_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(": ok") == 8 and "FAILED" not in r.stdout, r.stdout
