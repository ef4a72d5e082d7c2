"""The positive-part run of the Lanczos engine (full_eig! served by it) and its per-call certificate against exact checks
(proxsdp_hip_positive_part: Solver::lanczos(W, xp, nev, true) through the per-cycle observer, then Solver::lanczos_certificate on
the run's result or on given locked pairs, as Solver::full_eig_by_lanczos runs them).

  a  every cycle of a positive-part run (Krylov dimension 29, 128, 218 and a clipped 41; step kernels and k_lz_block1) by
     test_lanczos_cycles.py's rule, unchanged
  b  what the run returns: count, values, the soundness of the acceptance (true residuals against the thresholds applied),
     the failure exits
  c  the weighted warm start: k_lz_warm_sum with the lam-power weights, its cap and its LDS table
  d  the certificate on given locked pairs: k_lz_measure<1 | 2> + k_lz_finish (column npos), the step kernels started at
     kfirst = npos with a zero coupling row, across 64 and 128 columns, npos = 0 (k_lz_begin), the operator form; theta_max,
     scale, the caller's decision on must-pass and must-fail spectra; what the call leaves in the Ritz-vector buffer
  e  run then certificate, the production order; the exact hazard of test_lanczos_served_full_eig_is_certified_on_every_call

Bounds: a kernel quantity may be MARGIN = 8 times what the plain fp64 reference gives from the same inputs, floor 8 x 2^-52
(lanczos_cycle_cases); every reference is NumPy (positive_part_cases), the truth long double.  The conditions of every case are
checked on the CPU by test_positive_part_host.py; measured values: profiles/positive_part.md (the lines printed here)."""
import time

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import lanczos_cycle_cases as L
import positive_part_cases as P

pytestmark = pytest.mark.gpu
LD = L.LD


def _positive_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


def _norm(v):
    v = np.asarray(v).astype(LD)
    return np.sqrt((v * v).sum())


def _options(**opts):
    o = B.default_options()
    for k, v in opts.items():
        B.set_option(o, k, v)
    return o


# ------------------------------------------------------------------------------------------------ a: cycles
@pytest.mark.parametrize("cs", P.RUN_CASES, ids=lambda c: c["id"])
def test_every_cycle_of_a_positive_part_run_is_a_krylov_schur_decomposition(cs):
    t0 = time.time()
    n, kd = cs["n"], cs["kd"]
    A, _, normA, _, _ = P.run_matrix(cs)
    got = P.capture_run(cs)
    cyc = got["cycles"]
    assert (got["krylovdim"], got["cap"], got["npad"]) == (kd, cs["cap"], 64 * ((n + 63) // 64))
    # condition: the run restarted, in the cycles of the fp64 reference run
    assert len(cyc) == cs["cycles"] >= 2, (len(cyc), cs["cycles"])
    assert np.all(got["untouched"]["info"] == -1) and np.all(got["untouched"]["V"] == B.SYM_SENTINEL)
    v0, v0mag = P.run_start(cs), 1.0
    if cs["rp"] > 0:
        _, _, F, lam, _, _, _ = P.operator_pieces(n, cs["npos"], cs["rp"])
        v0mag = P.warm_column(F, lam, 1.0, L.start(n))[1]
        assert got["warm"] and all(cy["fop"] == cy["K"] - cy["kfirst"] and cy["ell_in_lds"] for cy in cyc)
    failures, prev, reuse = [], None, None
    for c, cy in enumerate(cyc):
        K, kf, V = cy["K"], cy["kfirst"], cy["V"]
        assert cy["engine"] == cs["engine"] and cy["stop"] == 0 and K == kd
        assert (kf == 0) == (c == 0) and 0 <= kf < K
        assert _positive_zero(V[n:, :K + 1]), "padding rows"
        assert np.all(cy["alphas"][:kf] == B.SYM_SENTINEL) and np.all(cy["betas"][K:] == B.SYM_SENTINEL)
        assert np.all(cy["D"][kf:] == B.SYM_SENTINEL) and np.all(cy["f"][kf:] == B.SYM_SENTINEL)
        if c == 0:
            # (the fixed start vector; a warm start's column: test_weighted_warm_start_column's bound, 8 x 2^-52 sum |terms| here)
            assert np.all(np.abs(V[:n, 0] - v0) <= (L.FLOOR * v0mag if got["warm"] else 2.0 * np.spacing(np.abs(v0)))), "start column"
            assert not cy["speculated"] and not cy["merge_on_device"] and not cy["kept_compared"]
        else:
            assert np.array_equal(V[:, kf], prev["V"][:, prev["K"]]), "v_kfirst is the previous cycle's v_K"
            assert cy["speculated"] == (cs["engine"] != "block1" and c >= 2)
            assert cy["kept_compared"] == (cs["engine"] != "block1")
            assert cy["kept_differ"] == 0, "the cycle changed its kept columns"
        Vr, alr, ber = L.reference_cycle(A, V, kf, K)
        qk, reuse_k = L.quantities(A, normA, cy, reuse)
        qr, _ = L.quantities(A, normA, dict(kfirst=kf, K=K, V=Vr, alphas=alr, betas=ber, D=cy["D"], f=cy["f"]), reuse_k)
        reuse = reuse_k
        print("PP|a" + L.ratio_lines(cs["id"], c, cy, qk, qr))
        assert qk["beta_min"] > 0.0
        for q in L.QUANTITIES:
            if not qk[q] <= L.bound(qr[q]):
                failures.append((c + 1, q, qk[q], qr[q], L.bound(qr[q])))
        if c > 0:
            res = L.span_residual(prev["V"][:n], prev["K"], V[:n, :kf])
            if not res <= L.bound(qr["r2"]):
                failures.append((c + 1, "span", res, qr["r2"], L.bound(qr["r2"])))
        prev = cy
    assert not failures, failures
    # every cycle but the last went on, the last one ended the run: the rule on NumPy's Rayleigh quotient of the captured cycle
    for c, cy in enumerate(cyc):
        D, _, f = P.rayleigh(cy)
        dec = P.rule(D, f, cs["nev"], P.TOL, P.POSRES)
        assert dec["decision"] == ("accept" if c + 1 == len(cyc) else "go_on"), (c + 1, dec)
    print(f"PP|time a {cs['id']} {time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------ b: what the run returns
@pytest.mark.parametrize("cs", P.RUN_CASES + P.TOL_CASES, ids=lambda c: c["id"])
def test_the_run_returns_every_positive_pair_and_its_acceptance_is_sound(cs):
    t0 = time.time()
    n, npos = cs["n"], cs["npos"]
    A, _, normA, _, ev = P.run_matrix(cs)
    got = P.capture_run(cs)
    assert got["converged"] and got["count"] == npos == int((ev > 0).sum())
    assert got["numiter"] == len(got["cycles"]) == cs["cycles"] and got["warm"] == (cs["rp"] > 0)
    vals, Z = got["vals"], got["Z"]
    assert len(vals) == npos and np.all(np.diff(vals) < 0.0) and np.all(vals > 0.0)
    last = got["cycles"][-1]
    K = last["K"]
    D, U, f = P.rayleigh(last)
    assert np.abs(vals - D[:npos]).max() <= 1e-13 * K * normA
    dec = P.rule(D, f, cs["nev"], P.TOL, P.POSRES, cs.get("tol_rel", 0.0))
    assert dec["decision"] == "accept" and dec["count"] == npos and dec["jn"] == npos < K
    assert dec["tol_neg"] == max(P.TOL, P.POSRES * dec["scale"]) and dec["tol_pos"] == max(P.TOL, cs.get("tol_rel", 0.0) * dec["scale"])
    # soundness: a Ritz residual equals its coupling up to the cycle's R1 defect |A V - V Tbar|_F, all in long double
    Vl = last["V"][:n, :K + 1].astype(LD)
    AV = L.times_a(A, last["V"][:n, :K])
    Tb = L.tmatrix(K, last["kfirst"], last["D"], last["f"], last["alphas"], last["betas"])
    Rm = AV - Vl @ Tb
    defect = float(np.sqrt((Rm * Rm).sum()))
    assert _positive_zero(Z[n:]), "padding rows of the Ritz vectors"
    Zl = Z[:n].astype(LD)
    res = np.sqrt((((L.times_a(A, Z[:n]) - Zl * vals.astype(LD)) ** 2).sum(axis=0))).astype(np.float64)
    zneg = Vl[:, :K] @ U[:, npos].astype(LD)
    rneg = float(_norm(L.times_a(A, zneg.astype(np.float64)[:, None])[:, 0] - zneg * LD(D[npos])))
    print(f"PP|b {cs['id']} | cycles {len(got['cycles'])} | largest positive residual {res.max():.2e} (tol {dec['tol_pos']:.1e}, largest |f| "
          f"{np.abs(f[:npos]).max():.2e}) | deciding pair {D[npos]:.4f}: residual {rneg:.2e} (threshold {dec['tol_neg']:.1e}, |f| {abs(f[npos]):.2e}) | "
          f"R1 defect {defect:.2e}")
    assert np.all(res <= dec["tol_pos"] + defect), (res.max(), dec["tol_pos"], defect)
    assert rneg <= dec["tol_neg"] + defect
    print(f"PP|time b {cs['id']} {time.time() - t0:.2f} s")


def test_failure_exits_of_the_run():
    cs = P.TOO_MANY                                                      # 7 positive eigenvalues, nev = 5
    _, packed, _, _, _ = P.run_matrix(cs)
    got = B.positive_part(cs["n"], cs["nev"], cs["ws_rank"], P.MAX_CYCLES, packed=packed, options=_options(**cs["opts"]), cert_steps=P.STEPS)
    assert not got["converged"] and got["count"] == 0 and len(got["cycles"]) == 1 and len(got["vals"]) == 0
    D, _, f = P.rayleigh(got["cycles"][0])
    assert P.rule(D, f, cs["nev"], P.TOL, P.POSRES)["decision"] == "too_many"
    assert not got["cert"]["ran"] and got["cert"]["matvecs"] == 0            # nothing to certify
    cs = P.MAXITER                                                       # max_cycles = 1 where the first cycle cannot decide
    _, packed, _, _, _ = P.run_matrix(cs)
    got = B.positive_part(cs["n"], cs["nev"], cs["ws_rank"], 1, packed=packed, options=_options(**cs["opts"]))
    assert not got["converged"] and got["count"] == 0 and len(got["cycles"]) == 1
    D, _, f = P.rayleigh(got["cycles"][0])
    assert P.rule(D, f, cs["nev"], P.TOL, P.POSRES)["decision"] == "go_on"


# ------------------------------------------------------------------------------------------------ c: the weighted warm start
@pytest.mark.parametrize("cs", P.WARM_CASES, ids=lambda c: c["id"])
def test_weighted_warm_start_column(cs):
    t0 = time.time()
    n, rp = cs["n"], cs["rp"]
    support, values, F, lam = P.warm_pieces(n, rp, cs["lam_kind"])
    got = B.positive_part(n, cs["nev"], cs["ws_rank"], 1, operator=dict(support=support, values=values, F=F, lam=lam, f_first=cs["f_first"]),
                          options=_options(full_eig_lanczos_warm_pow=cs["wpow"], lanczos_warm_start=cs["warm"]))
    cy = got["cycles"][0]
    assert cy["stop"] == 0 and cy["kfirst"] == 0 and cy["K"] == got["krylovdim"] == 29 and cy["fop"] == 29      # control block cleared
    col = cy["V"][:, 0]
    assert np.all(np.isfinite(col)) and _positive_zero(col[n:]), "finite, padding rows"
    r0 = L.start(n)
    assert abs(float(_norm(col)) - 1.0) <= L.FLOOR
    if cs["warm"] < 0:
        # switched off: the fixed start vector -- the bits k_lz_begin gives a packed run of the same side (a hand-over check
        # between two device runs), and the vector itself within the 2 ulp of the library's own normalisation, as in test a
        assert not got["warm"]
        cold = P.capture_run(next(c for c in P.RUN_CASES if c["n"] == n and c["engine"] == "step"))["cycles"][0]["V"][:, 0]
        assert col.tobytes() == cold.tobytes()
        assert np.all(np.abs(col[:n] - r0) <= 2.0 * np.spacing(np.abs(r0)))
        print(f"PP|c {cs['id']} | no weights: the fixed start vector bit for bit, largest |column - start| / ulp "
              f"{float((np.abs(col[:n] - r0) / np.spacing(np.abs(r0))).max()):.1f} | {time.time() - t0:.2f} s")
        return
    assert got["warm"]
    want, mag = P.warm_column(F, lam, cs["wpow"], r0, LD)
    c64, _ = P.warm_column(F, lam, cs["wpow"], r0)
    err = np.abs(col[:n].astype(LD) - want).astype(np.float64)
    ref = np.abs(c64.astype(LD) - want).astype(np.float64)
    bnd = np.maximum(L.MARGIN * ref, L.FLOOR * mag.astype(np.float64))
    w = P.warm_weights(lam, cs["wpow"])
    print(f"PP|c {cs['id']} | weights {w.min():.3g} .. {w.max():.3g} | largest error / bound {float((err / bnd).max()):.3f} | "
          f"largest error / (2^-52 sum |terms|) {float((err / (L.EPS * mag.astype(np.float64))).max()):.3f} | {time.time() - t0:.2f} s")
    assert np.all(err <= bnd), float((err / bnd).max())


# ------------------------------------------------------------------------------------------------ d: the certificate
def _certificate_checks(tag, A, normA, n, Z, vals, cert, msteps, given=True):
    """what Solver::lanczos_certificate computed and left behind, for locked pairs (Z, vals) and msteps steps"""
    npos, K = Z.shape[1], Z.shape[1] + msteps
    assert cert["ran"] and cert["npos"] == npos and cert["steps"] == msteps and cert["stop"] == 0 and cert["matvecs"] == msteps
    basis, r2 = cert["basis"], cert["resid2"]
    # ---- the second start vector
    assert abs(float(_norm(r2)) - 1.0) <= L.FLOOR and _positive_zero(r2[n:])
    assert np.array_equal(r2[:n], P.resid2(n))
    cos = abs(float(r2[:n] @ L.start(n)))
    assert cos < 0.5, cos
    # ---- what the call leaves behind
    assert cert["differ"] == 0
    assert np.array_equal(basis[:n, :npos], Z) and np.all(basis[:, K + 1:] == B.SYM_SENTINEL)
    assert _positive_zero(basis[n:, :K + 1]), "padding rows"
    # ---- column npos = (r2 - Z Z'r2) / |.|: k_lz_measure + k_lz_finish (npos = 0: k_lz_begin's copy)
    want = P.start_column(Z, r2[:n], LD)
    err = float(np.abs(basis[:n, npos].astype(LD) - want).max())
    ref = float(np.abs(P.start_column(Z, r2[:n]).astype(LD) - want).max())
    assert err <= L.bound(ref), (err, ref)
    if npos == 0:
        assert np.array_equal(basis[:, 0], r2)
    # ---- the columns npos .. npos + msteps by the rule of the cycles
    al, be = cert["alphas"], cert["betas"]
    assert np.all(al[:npos] == B.SYM_SENTINEL) and np.all(be[K:] == B.SYM_SENTINEL)
    cyc = dict(kfirst=npos, K=K, V=basis, alphas=al, betas=be, D=vals, f=np.zeros(npos))
    Vr, alr, ber = L.reference_cycle(A, basis, npos, K)
    qk, reuse = L.quantities(A, normA, cyc)
    qr, _ = L.quantities(A, normA, dict(cyc, V=Vr, alphas=alr, betas=ber), reuse)
    assert qk["beta_min"] > 0.0
    bad = [(q, qk[q], qr[q]) for q in L.QUANTITIES if not qk[q] <= L.bound(qr[q])]
    assert not bad, bad
    # ---- theta_max and scale
    theta, floor = cert["theta_max"], 1e-13 * msteps * normA
    T = np.diag(al[npos:K]) + np.diag(be[npos:K - 1], 1) + np.diag(be[npos:K - 1], -1)
    assert abs(theta - np.linalg.eigvalsh(T)[-1]) <= floor
    # (an equality of bits needs the library's own host eigensolver for d_0, the routine lanczos_certificate calls: this line
    # checks how scale is put together, not the eigensolver -- theta_max is held to NumPy's eigvalsh above)
    d, _ = B.host_symeig(T)
    assert cert["scale"] == P.cert_scale(theta, d[0], vals)
    tl = float(P.certificate_reference(A, Z, vals, r2[:n], msteps, dtype=LD)["theta_max"])
    t64 = P.certificate_reference(A, Z, vals, r2[:n], msteps)["theta_max"]
    assert abs(theta - tl) <= max(L.MARGIN * abs(t64 - tl), floor), (theta, tl, t64)
    top = P.complement_max(A, Z)
    assert theta <= top + floor
    ratios = " ".join(f"{qk[q] / max(qr[q], L.EPS):.2f}" for q in L.QUANTITIES)
    print(f"PP|d {tag} | NCH {P.nch(max(npos, 1))} -> {P.nch(K)} | column npos {err:.2e} / {ref:.2e} = {err / max(ref, L.EPS):.2f} | "
          f"{ratios} | theta_max {theta:.6f} (long double {tl:.6f}, |diff| {abs(theta - tl):.1e}; complement {top:.4f}) | scale {cert['scale']:.4f} | "
          f"mat-vecs {cert['matvecs']}")
    return P.decision(theta, cert["scale"], cert["posres"])


def _certificate(cs, **kw):
    A, block, normA, Z, vals = P.cert_inputs(cs)
    got = B.positive_part(cs["n"], cs["nev"], cs["ws_rank"], 1, run=False, cert_steps=cs["steps"], locked=Z, locked_vals=vals, **block, **kw)
    assert got["cycles"] == [] and not got["converged"] and got["count"] == 0
    return A, normA, Z, vals, got


@pytest.mark.parametrize("cs", P.CERT_CASES, ids=lambda c: c["id"])
def test_certificate_on_given_locked_pairs(cs):
    t0 = time.time()
    A, normA, Z, vals, got = _certificate(cs)
    cert = got["cert"]
    assert cert["posres"] == P.POSRES and got["cap"] == 256
    passed = _certificate_checks(cs["id"], A, normA, cs["n"], Z, vals, cert, cs["steps"])
    assert passed == cs["must_pass"], (cert["theta_max"], cert["scale"])
    if cs["kind"] == "hidden7":
        assert abs(cert["theta_max"] - 7.0) <= P.HIDDEN7
    # the same bits on a second call
    again = _certificate(cs)[4]["cert"]
    for key in ("resid2", "basis", "alphas", "betas"):
        assert again[key].tobytes() == cert[key].tobytes(), key
    assert (again["theta_max"], again["scale"]) == (cert["theta_max"], cert["scale"])
    print(f"PP|time d {cs['id']} {time.time() - t0:.2f} s")


def test_certificate_with_a_complement_smaller_than_its_steps():
    """n = 72, 64 locked pairs, ten steps in the 8 directions that are left, the hidden 7 among them: the recurrence runs out of
    directions; a must-fail case stays must-fail"""
    cs = P.SMALL_COMPLEMENT
    A, normA, Z, vals, got = _certificate(cs)
    cert = got["cert"]
    print(f"PP|d {cs['id']} | ran {cert['ran']} steps {cert['steps']} stop {cert['stop']} kstop {cert['kstop']} theta_max {cert['theta_max']:.6f} "
          f"scale {cert['scale']:.4f} | betas {np.array2string(cert['betas'][64:74], precision=2)}")
    assert cert["differ"] == 0
    assert (not cert["ran"]) or (np.isfinite(cert["theta_max"]) and not P.decision(cert["theta_max"], cert["scale"], cert["posres"]))


def test_certificate_refuses_a_workspace_that_is_too_small():
    cs = P.TOO_SMALL
    A, normA, Z, vals, got = _certificate(cs)
    cert = got["cert"]
    assert got["cap"] == 42 and not cert["ran"] and cert["npos"] == 32 and cert["matvecs"] == 0 and cert["differ"] == 0
    for key in ("basis", "resid2", "alphas", "betas"):
        assert np.all(cert[key] == B.SYM_SENTINEL), key


# ------------------------------------------------------------------------------------------------ e: run, then certificate
@pytest.mark.parametrize("cs", P.E_CASES, ids=lambda c: c["id"])
def test_a_converged_run_is_certified_and_keeps_its_result(cs):
    t0 = time.time()
    n = cs["n"]
    A, _, normA, _, _ = P.run_matrix(cs)
    got = P.capture_run(cs)
    assert got["converged"] and got["count"] == cs["npos"] and got["cycles"][-1]["engine"] == cs["engine"]
    passed = _certificate_checks(cs["id"] + "-own", A, normA, n, got["Z"][:n], got["vals"], got["cert"], P.STEPS)
    assert passed, (got["cert"]["theta_max"], got["cert"]["scale"])
    assert np.array_equal(got["cert"]["basis"][:, :cs["npos"]], got["Z"])          # (padding rows included)
    print(f"PP|time e {cs['id']} {time.time() - t0:.2f} s")


def test_the_certificate_finds_what_a_deficient_start_vector_hides():
    """the exact hazard of test_lanczos_served_full_eig_is_certified_on_every_call: the run converges with a count short by three
    (7 and two copies of 5 are invisible to its Krylov space), the certificate's vector sees them"""
    t0 = time.time()
    A, packed, lam, deficient, nev = P.hazard()
    n = A.shape[0]
    got = B.positive_part(n, nev, 46, P.MAX_CYCLES, packed=packed, resid=deficient, cert_steps=P.STEPS)
    assert got["converged"] and got["count"] == nev == int((lam > 0).sum()) - 3
    assert np.abs(got["vals"] - np.array([9.0, 5.0, 3.0, 1.0])).max() <= 1e-9
    cert = got["cert"]
    passed = _certificate_checks("hazard-n257", A, 9.0, n, got["Z"][:n], got["vals"], cert, P.STEPS)
    assert not passed and abs(cert["theta_max"] - 7.0) <= P.HIDDEN7, cert["theta_max"]
    print(f"PP|time e hazard {time.time() - t0:.2f} s")



# ------------------------------------------------------------------------------------------------ a record, no assertion
def test_record_theta_max_on_a_small_hidden_eigenvalue():
    """what ten steps do and do not detect: one positive eigenvalue of 1e-3 and of 1e-5 times the scale outside the locked pairs,
    n = 257, npos = 17 and 64, five matrices each.  The plain fp64 recurrence finds theta_max anywhere between the bulk and that
    value, so nothing is asserted of it: the device's value and the reference's are printed for profiles/positive_part.md."""
    n = 257
    for tiny in (1e-3, 1e-5):
        for npos in (17, 64):
            for seed in range(5):
                A, packed, normA, Q, ev = P.spectrum(n, npos, seed=seed, tiny=tiny)
                Z, vals = Q[:, :npos], ev[:npos]
                cert = B.positive_part(n, 7, 127, 1, packed=packed, run=False, cert_steps=P.STEPS, locked=Z, locked_vals=vals)["cert"]
                ref = P.certificate_reference(A, Z, vals, P.resid2(n), P.STEPS)["theta_max"]
                assert cert["ran"] and np.isfinite(cert["theta_max"])
                print(f"PP|obs | {tiny:g} | {npos} | {seed} | {ev[npos]:.3e} | {cert['theta_max']:.6e} | {ref:.6e} | "
                      f"{'passes' if P.decision(cert['theta_max'], cert['scale'], cert['posres']) else 'fails'} |")
