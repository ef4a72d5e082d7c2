"""Cases, spectra and plain references of the tests of the positive-part Lanczos run and its per-call certificate
(test_positive_part.py on the GPU, test_positive_part_host.py on the CPU).  The per-cycle checks, the plain fp64 reference cycle,
MARGIN and the floors are lanczos_cycle_cases'; the operator form is operator_cycle_cases.Operator.

Spectra (`spectrum`): A = Q diag(ev) Q' with Q from a seeded QR, npos positive values linspace(9, 1, npos), optionally hidden
values (7, or 5, 5, 5) that a locked set leaves out, the rest a bulk in [-3, -0.5]: nothing lies within 1e-3 x 9 of zero and
only a case that says so has exact duplicates.

The certificate (`certificate_reference`): v = (r2 - Z Z'r2) / |.|, then msteps Lanczos steps with two measured classical
Gram-Schmidt passes against ALL columns (the locked ones included), theta_max = the largest eigenvalue of the msteps x msteps
tridiagonal -- in fp64 (the yardstick) and in long double (the truth).  What the reference gives on n in {130, 257, 520}, npos
in {0, 1, 16, 17, 63, 64, 65, 100}, 5 seeds, 10 steps: theta_max in [-0.61, -0.50] when everything left is <= -0.5; 7.000 to
four digits with a hidden 7; anywhere in [-0.11, 1e-3] with a hidden 1e-3 (ten steps do not promise to find a small isolated
positive value: recorded in profiles/positive_part.md, asserted nowhere).

The acceptance (`rule`): lz_after_cycle's decision for a positive-part run, from its comment: all positive Ritz pairs converged
to tol (or to tol_rel x the spectral scale) AND the first strictly negative pair resolved to max(tol, posres x scale)."""
import functools
import math

import numpy as np

import lanczos_cycle_cases as L
import operator_cycle_cases as O
from proxsdp_jl_amd.state_io import svec

LD = L.LD
EPS = L.EPS
SEED = 41500
TOL = 1e-12                                        # krylovkit_tol
POSRES = 1e-6                                      # lanczos_posres() at the default tolerances
KDIM10 = 30
MIN_LANCZOS = 25                                   # eigsolver_min_lanczos
STEPS = 10                                         # full_eig_lanczos_certify's default
CLEAN = (-0.61, -0.50)                             # theta_max of the reference when everything left is <= -0.5
HIDDEN7 = 5e-4                                     # |theta_max - 7| of the reference with a hidden 7 ("7.000 to four digits")


# ------------------------------------------------------------------------------------------------ dimensions
def dims(n, nev, ws_rank, min_lanczos=MIN_LANCZOS, kdim10=KDIM10):
    """(cap, krylovdim) of a positive-part run as include/proxsdp_hip.h states them"""
    cap = min(max(2 * min(max(ws_rank, 2), n) + 1, min_lanczos), 255) + 1
    return cap, min(min(cap, 256) - 1, max(max(2 * nev + 1, min_lanczos), nev * kdim10 // 10 + 8))


def nch(cols):
    """the 64-column chunks a step kernel is built for (solver.hip.hpp lz_nch)"""
    return 1 if cols <= 64 else 2 if cols <= 128 else 3 if cols <= 192 else 4


# ------------------------------------------------------------------------------------------------ spectra
@functools.lru_cache(maxsize=None)
def spectrum(n, npos, seed=0, hidden=(), tiny=None, edge=0):
    """(A, packed, normA, Q, ev): ev = linspace(9, 1, npos), then `hidden`, then (tiny: one value tiny x 9) the bulk, uniform in
    [-3, -0.5] -- its first `edge` values packed at the upper end, linspace(-0.5, -0.52, edge): distinct values that a Krylov
    space of most of the side still needs a restart to resolve; the eigenvector of ev[i] is Q[:, i]"""
    rng = np.random.default_rng(SEED + 1000 * n + 10 * npos + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    extra = list(hidden) + ([tiny * 9.0] if tiny is not None else [])
    ev = np.concatenate([np.linspace(9.0, 1.0, npos), extra, np.linspace(-0.5, -0.52, edge),
                         rng.uniform(-3.0, -0.5, n - npos - len(extra) - edge)])
    A = (Q * ev) @ Q.T
    A = (A + A.T) / 2
    for a in (A, Q, ev):
        a.setflags(write=False)
    return A, svec(A), float(np.abs(ev).max()), Q, ev


@functools.lru_cache(maxsize=None)
def operator_pieces(n, npos, rp, seed=0, hidden=0.0):
    """the operator form A = F diag(lam) F' + E with a known count of positive eigenvalues: E = -1.75 I + 1.25 E0 / |E0|_2 on the
    sparse pattern (every eigenvalue in [-3, -0.5]), F orthonormal, lam = linspace(12, 4, npos) (+ `hidden` = 10 on one more
    column when asked for) and 0.3 on the other columns.  By Weyl's inequalities exactly npos (+ 1) eigenvalues are positive,
    each >= 1, and every other one is <= -0.2.  Returns (support, values, F, lam, normA, w, U): eigh of the dense matrix,
    descending."""
    rng = np.random.default_rng(SEED + 7919 * n + 101 * npos + 13 * rp + seed)
    support = O.pattern_sparse(n, rng)
    i, j = O.unpacked_index(support)
    values = rng.standard_normal(len(support)) * np.where(i == j, 1.0, math.sqrt(2.0))
    E0 = O.Operator(n, support, values, np.zeros((n, 0)), np.zeros(0)).dense_e()
    values = 1.25 * values / np.abs(np.linalg.eigvalsh(E0)).max()
    values[i == j] -= 1.75
    F, _ = np.linalg.qr(rng.standard_normal((n, rp)))
    big = np.concatenate([np.linspace(12.0, 4.0, npos), [10.0] if hidden else []])
    assert len(big) <= rp
    lam = np.concatenate([big, np.full(rp - len(big), 0.3)])
    A = O.Operator(n, support, values, F, lam)
    w, U = np.linalg.eigh(A.dense())
    w, U = w[::-1].copy(), U[:, ::-1].copy()
    for a in (support, values, F, lam, w, U):
        a.setflags(write=False)
    return support, values, F, lam, float(np.abs(w).max()), w, U


def matvec(A, v, dtype):
    if dtype is np.float64:
        return A @ v
    if hasattr(A, "times_ld"):
        return A.times_ld(np.asarray(v, dtype=np.float64)[:, None])[:, 0] if v.dtype == np.float64 else _times_ld_vec(A, v)
    return A.astype(LD) @ v


def _times_ld_vec(A, v):
    """Operator.times_ld takes fp64 columns; a long double vector goes through its pieces"""
    out = A.Fld @ (A.lamld * (A.Fld.T @ v))
    np.add.at(out, A.rows, A.eld * v[A.cols])
    return out


# ------------------------------------------------------------------------------------------------ the certificate
def start_column(Z, r2, dtype=np.float64):
    """(r2 - Z Z'r2) / |.|"""
    Zt, r = np.asarray(Z).astype(dtype), np.asarray(r2).astype(dtype)
    v = r - Zt @ (Zt.T @ r)
    return v / np.sqrt((v * v).sum())


def tridiag_max(al, be, dtype=np.float64):
    """the largest eigenvalue of tridiag(al, be[:-1]): eigvalsh in fp64, bisection on the Sturm count in long double"""
    m = len(al)
    if dtype is np.float64:
        T = np.diag(al) + np.diag(be[:m - 1], 1) + np.diag(be[:m - 1], -1)
        return float(np.linalg.eigvalsh(T)[-1])
    al, be = np.asarray(al, dtype=LD), np.asarray(be, dtype=LD)
    r = np.abs(al).max() + 2 * (np.abs(be[:m - 1]).max() if m > 1 else LD(0))
    lo, hi = -r, r

    def below(x):                                  # eigenvalues < x
        cnt, q = 0, LD(1)
        for k in range(m):
            q = al[k] - x - (be[k - 1] ** 2 / q if k > 0 else LD(0))
            if q == 0:
                q = np.finfo(LD).tiny
            cnt += q < 0
        return cnt
    for _ in range(90):
        mid = (lo + hi) / 2
        if below(mid) >= m:
            hi = mid
        else:
            lo = mid
    return (lo + hi) / 2


def certificate_reference(A, Z, vals, r2, msteps, dtype=np.float64, v0=None):
    """the certificate's recurrence, plainly: v = (r2 - Z Z'r2) / |.| (or v0, the column a device run produced), msteps steps of
    w = A v_k with two measured classical Gram-Schmidt passes against all npos + k + 1 columns, theta_max of the tridiagonal.
    Returns dict(V (n, npos + msteps + 1), alphas, betas (at their step's index), theta_max, steps)."""
    n = A.shape[0]
    Z = np.asarray(Z).reshape(n, -1)
    npos = Z.shape[1]
    V = np.zeros((n, npos + msteps + 1), dtype=dtype)
    V[:, :npos] = Z
    V[:, npos] = start_column(Z, r2, dtype) if v0 is None else np.asarray(v0)[:n]
    al, be = np.zeros(npos + msteps, dtype=dtype), np.zeros(npos + msteps, dtype=dtype)
    steps = msteps
    for k in range(npos, npos + msteps):
        w = matvec(A, V[:, k], dtype)
        B = V[:, :k + 1]
        h1 = B.T @ w
        w = w - B @ h1
        h2 = B.T @ w
        w = w - B @ h2
        al[k] = h1[k] + h2[k]
        be[k] = np.sqrt((w * w).sum())
        if not be[k] > 0:
            steps = k + 1 - npos
            break
        V[:, k + 1] = w / be[k]
    return dict(V=V, alphas=al, betas=be, steps=steps, theta_max=tridiag_max(al[npos:npos + steps], be[npos:npos + steps], dtype))


def complement_max(A, Z):
    """lambda_max of A restricted to the orthogonal complement of span(Z): what theta_max is a lower bound of"""
    n = A.shape[0]
    Ad = A.dense() if hasattr(A, "dense") else np.asarray(A)
    Z = np.asarray(Z).reshape(n, -1)
    if Z.shape[1] == 0:
        return float(np.linalg.eigvalsh(Ad)[-1])
    Qf, _ = np.linalg.qr(Z, mode="complete")
    C = Qf[:, Z.shape[1]:]
    return float(np.linalg.eigvalsh(C.T @ Ad @ C)[-1])


def resid2(n):
    """the certificate's second start vector as the library draws it (start_vector, seed 1234 ^ 0x9e3779b97f4a7c15, rule 3)"""
    from proxsdp_jl_amd import binding as B
    seed = (1234 ^ 0x9e3779b97f4a7c15)
    return B.host_start_vector(n, seed - (1 << 64) if seed >= (1 << 63) else seed, 3)


# ------------------------------------------------------------------------------------------------ the acceptance rule
def rule(D, f, nev, tol, posres, tol_rel=0.0):
    """lz_after_cycle's decision for a positive-part run on the Ritz values D (descending) and couplings f of a K-column cycle.
    Returns dict(decision: "accept" | "too_many" | "go_on", count, converged, jn, scale, tol_pos, tol_neg): count = the
    positive Ritz values, jn = the first strictly negative one (K: none), tol_pos / tol_neg the thresholds applied."""
    D, f = np.asarray(D, dtype=np.float64), np.asarray(f, dtype=np.float64)
    K = len(D)
    scale = max(abs(D[0]), abs(D[K - 1]))
    tol_pos = max(tol, tol_rel * scale) if tol_rel > 0.0 else tol
    conv = 0
    while conv < K and abs(f[conv]) <= tol_pos:
        conv += 1
    j = 0
    while j < K and D[j] > 0.0:
        j += 1
    jn = j
    while jn < K and D[jn] >= -1e-12 * scale:
        jn += 1
    tol_neg = max(tol, posres * scale)
    out = dict(count=j, converged=conv, jn=jn, scale=scale, tol_pos=tol_pos, tol_neg=tol_neg)
    if j > nev:
        return dict(out, decision="too_many")
    if conv >= j and (jn == K or abs(f[jn]) <= tol_neg):
        return dict(out, decision="accept")
    return dict(out, decision="go_on")


def rayleigh(cyc):
    """(D descending, U, f) of a captured cycle's Rayleigh quotient, by NumPy from its arrow and coefficients"""
    K = cyc["K"]
    T = L.tmatrix(K, cyc["kfirst"], cyc["D"], cyc["f"], cyc["alphas"], cyc["betas"], np.float64)[:K, :K]
    w, U = np.linalg.eigh((T + T.T) / 2)
    D, U = w[::-1].copy(), U[:, ::-1].copy()
    return D, U, cyc["betas"][K - 1] * U[K - 1, :]


def reference_run(A, v0, nev, kd, max_cycles, tol=TOL, posres=POSRES, tol_rel=0.0):
    """the positive-part run in plain fp64: lanczos_cycle_cases.reference_cycle, `rule`, the Krylov-Schur restart with
    keep = (3 kd + 2 converged) // 5.  Returns (cycles, the last decision's dict with "decision" = "maxiter" when the run
    used max_cycles without a decision)."""
    n = A.shape[0]
    V = np.zeros((n, kd + 1))
    V[:, 0] = v0 / np.linalg.norm(v0)
    kfirst, D, f = 0, np.zeros(0), np.zeros(0)
    out = []
    for c in range(max_cycles):
        V, al, be = L.reference_cycle(A, V, kfirst, kd)
        cyc = dict(kfirst=kfirst, K=kd, V=V.copy(), alphas=al, betas=be, D=D, f=f)
        out.append(cyc)
        Dd, U, ff = rayleigh(cyc)
        dec = rule(Dd, ff, nev, tol, posres, tol_rel)
        if dec["decision"] != "go_on":
            return out, dec
        if c + 1 == max_cycles:
            return out, dict(dec, decision="maxiter")
        keep = (3 * kd + 2 * dec["converged"]) // 5
        Vn = np.zeros_like(V)
        Vn[:, :keep] = V[:, :kd] @ U[:, :keep]
        Vn[:, keep] = V[:, kd]
        V, D, f, kfirst = Vn, Dd[:keep].copy(), ff[:keep].copy(), keep
    raise AssertionError("unreachable")


# ------------------------------------------------------------------------------------------------ cases: the run (a, b, e)
def run_case(n, npos, nev, ws_rank, engine, tag, cycles, edge=0, rp=0, tight=False, **opts):
    """rp > 0: the operator form with rp factor columns (operator_pieces), started warm as a positive-part run is by default;
    tight: tight_spectrum, whose positive pairs converge last"""
    cap, kd = dims(n, nev, ws_rank)
    return dict(n=n, npos=npos, nev=nev, ws_rank=ws_rank, cap=cap, kd=kd, engine=engine, cycles=cycles, edge=edge, rp=rp, tight=tight,
                opts=dict(opts), id=f"n{n}-npos{npos}-nev{nev}-K{kd}-{tag}")


STEP, B1 = dict(lanczos_cycle_kernel=0), dict(lanczos_cycle_kernel=2)
MAX_CYCLES = 12
# n, positive eigenvalues, nev, workspace rank, the engine lz_plan must choose, tag, the cycles of the run (those of the fp64
# reference run: test_positive_part_host.py holds the table to it; every run restarts at least once), the bulk values packed
# at its upper edge.  Krylov dimension max(25, 2 nev + 1, 3 nev + 8), clipped to cap - 1 in the "clipped" case.
RUN_CASES = [
    run_case(130, 5, 7, 127, "step", "step", 5, **STEP),                  # krylovdim 29: NCH 1
    run_case(130, 5, 7, 127, "block1", "block1", 5, **B1),
    # (a packed triangle of side 257 does not fit the LDS of k_lz_block1: there the one-workgroup kernel runs the operator form)
    run_case(257, 5, 7, 127, "block1", "operator-block1", 3, rp=8, **B1),   # two row groups a wave, E in LDS, warm start
    run_case(257, 30, 40, 127, "step", "step", 3, edge=30),               # krylovdim 128: NCH 2, keep 88; the restart's basis has 129 columns
    run_case(257, 60, 70, 127, "step", "step", 2, edge=30),               # krylovdim 218: NCH 4, keep 154
    run_case(130, 12, 20, 20, "step", "clipped", 2, **STEP),              # cap 42: krylovdim 41 = cap - 1 (unclipped: 68)
]
# the tolerance of the positive pairs decides: two of them 5e-4 apart, the first negative eigenvalue isolated.  At the end of the
# first cycle the pair's couplings are a few 1e-12 -- above krylovkit_tol = 1e-12, below full_eig_lanczos_tol = 1e-9 x scale
TIGHT_CASE = run_case(130, 6, 7, 127, "step", "tight", 2, tight=True, **STEP)
TOL9_CASE = dict(run_case(130, 6, 7, 127, "step", "tight-tol1e-9", 1, tight=True, full_eig_lanczos_tol=1e-9, **STEP), tol_rel=1e-9)
TOL_CASES = [TIGHT_CASE, TOL9_CASE]
E_CASES = [RUN_CASES[2], RUN_CASES[4]]
# failure exits: more positive Ritz values than nev (7 positive eigenvalues, nev = 5); maxiter (the first cycle cannot decide)
TOO_MANY = dict(run_case(130, 7, 5, 127, "step", "too-many", 1, **STEP))
MAXITER = dict(RUN_CASES[0], id=RUN_CASES[0]["id"] + "-maxiter")


def run_matrix(cs):
    """(A, packed or None, normA, Q or None, ev) of a run case: a dense matrix, or an Operator"""
    if cs["tight"]:
        return tight_spectrum(cs["n"])
    if cs["rp"] == 0:
        return spectrum(cs["n"], cs["npos"], edge=cs["edge"])
    support, values, F, lam, normA, w, _ = operator_pieces(cs["n"], cs["npos"], cs["rp"])
    return O.Operator(cs["n"], support, values, F, lam), None, normA, None, w


@functools.lru_cache(maxsize=None)
def tight_spectrum(n):
    """spectrum's layout with ev = 9, 6.67, 4.33, 2, 1.0005, 1, then -0.5 alone, the rest uniform in [-3, -1.2]"""
    rng = np.random.default_rng(SEED + 5 * n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.concatenate([np.linspace(9.0, 2.0, 4), [1.0005, 1.0], [-0.5], rng.uniform(-3.0, -1.2, n - 7)])
    A = (Q * ev) @ Q.T
    A = (A + A.T) / 2
    for a in (A, Q, ev):
        a.setflags(write=False)
    return A, svec(A), 9.0, Q, ev


def run_start(cs):
    """the run's start vector: the fixed one, or -- operator form -- the weighted warm start (fp64)"""
    if cs["rp"] == 0:
        return L.start(cs["n"])
    _, _, F, lam, _, _, _ = operator_pieces(cs["n"], cs["npos"], cs["rp"])
    return warm_column(F, lam, 1.0, L.start(cs["n"]))[0]


def _options(opts):
    from proxsdp_jl_amd import binding as B
    o = B.default_options()
    for k, v in opts.items():
        B.set_option(o, k, v)
    return o


@functools.lru_cache(maxsize=None)
def _captured(key):
    from proxsdp_jl_amd import binding as B
    cs = next(c for c in RUN_CASES + TOL_CASES if c["id"] == key)
    _, packed, _, _, _ = run_matrix(cs)
    if packed is not None:
        block = dict(packed=packed)
    else:
        support, values, F, lam, _, _, _ = operator_pieces(cs["n"], cs["npos"], cs["rp"])
        block = dict(operator=dict(support=support, values=values, F=F, lam=lam))
    return B.positive_part(cs["n"], cs["nev"], cs["ws_rank"], MAX_CYCLES, options=_options(cs["opts"]), cert_steps=STEPS, **block)


def capture_run(cs):
    """the case's run and the certificate of its own result through proxsdp_hip_positive_part, once for all tests (GPU)"""
    return _captured(cs["id"])


# ------------------------------------------------------------------------------------------------ cases: the warm start (c)
def warm_case(n, rp, f_first=0, wpow=1.0, lam_kind="plain", warm=0):
    return dict(n=n, rp=rp, f_first=f_first, wpow=wpow, lam_kind=lam_kind, warm=warm, nev=7, ws_rank=127,
                id=f"n{n}-rp{rp}-first{f_first}-pow{wpow}-{lam_kind}" + ("-off" if warm < 0 else ""))


WARM_CASES = ([warm_case(257, rp) for rp in (1, 5, 64, 65, 127)] + [warm_case(130, 5), warm_case(130, 127)] +
              [warm_case(257, 5, f_first=40), warm_case(257, 65, f_first=40)] +
              [warm_case(257, rp, wpow=w) for rp in (5, 65) for w in (0.5, 0.0)] +
              [warm_case(257, rp, lam_kind=k) for rp in (5, 65) for k in ("small", "denormal")] +
              [warm_case(257, 5, warm=-1)])


@functools.lru_cache(maxsize=None)
def warm_pieces(n, rp, lam_kind):
    """(support, values, F, lam): E on the sparse pattern with its spectrum in [-3, -0.5], F orthonormal, lam = linspace(9, 1, rp);
    "small": one lam at 1e-9 lam_0, "denormal": one at 1e-310 -- the cap 1e6 decides their weight"""
    support, values, _, _, _, _, _ = operator_pieces(n, 0, 1)
    rng = np.random.default_rng(SEED + 31 * n + rp)
    F, _ = np.linalg.qr(rng.standard_normal((n, rp)))
    lam = np.linspace(9.0, 1.0, rp) if rp > 1 else np.array([9.0])
    if lam_kind == "small":
        lam[rp // 2] = 1e-9 * lam[0]
    elif lam_kind == "denormal":
        lam[rp // 2] = 1e-310
    F.setflags(write=False)
    lam.setflags(write=False)
    return support, values, F, lam


def warm_weights(lam, wpow, dtype=np.float64):
    """k_lz_warm_sum's weights: min(lam_0 / lam_c, 1e6)^wpow (1 when wpow = 0)"""
    lam = np.asarray(lam).astype(dtype)
    if wpow == 0.0:
        return np.ones(len(lam), dtype=dtype)
    with np.errstate(over="ignore"):
        return np.minimum(lam[0] / lam, dtype(1e6)) ** dtype(wpow)


def warm_column(F, lam, wpow, r, dtype=np.float64):
    """((sum_c w_c F_c + 1e-3 r) / |.|, sum of the terms' magnitudes / |.|) in the given precision"""
    w = warm_weights(lam, wpow, dtype)
    Ft, rt = np.asarray(F).astype(dtype) * w, dtype(1e-3) * np.asarray(r).astype(dtype)
    v = Ft.sum(axis=1) + rt
    s = np.sqrt((v * v).sum())
    return v / s, (np.abs(Ft).sum(axis=1) + np.abs(rt)) / s


# ------------------------------------------------------------------------------------------------ cases: the certificate (d)
def cert_case(n, npos, steps=STEPS, kind="clean", form="packed", rp=0):
    """kind: "clean" (everything left <= -0.5: must pass), "hidden7", "hidden555" (values outside the locked set: must fail),
    "short" (the last positive pair is not locked: must fail)"""
    return dict(n=n, npos=npos, steps=steps, kind=kind, form=form, rp=rp, nev=7, ws_rank=127, must_pass=kind == "clean",
                id=f"{form}-n{n}-npos{npos}-m{steps}-{kind}" + (f"-rp{rp}" if form == "operator" else ""))


NPOS = (0, 1, 16, 17, 60, 63, 64, 65, 100)
CERT_CASES = ([cert_case(n, npos) for n in (130, 257) for npos in NPOS] +
              [cert_case(130, 17, 2), cert_case(257, 17, 2), cert_case(130, 60, 30), cert_case(257, 60, 30), cert_case(257, 100, 30)] +
              [cert_case(257, npos, kind="hidden7") for npos in (0, 17, 60, 64)] + [cert_case(130, 17, kind="hidden7")] +
              [cert_case(257, 17, kind="hidden555"), cert_case(130, 60, kind="hidden555"), cert_case(257, 63, kind="short")] +
              [cert_case(520, 65), cert_case(520, 17, kind="hidden7")] +
              # operator form: the owner form of F'v (rp <= 2 nt) and the records form, one and two chunks of factor columns
              [cert_case(257, 0, form="operator", rp=5), cert_case(257, 0, form="operator", rp=70),
               cert_case(257, 17, form="operator", rp=20), cert_case(257, 17, form="operator", rp=70),
               cert_case(257, 60, form="operator", rp=64), cert_case(257, 60, form="operator", rp=65),
               cert_case(130, 65, form="operator", rp=66), cert_case(257, 65, form="operator", rp=127),
               cert_case(257, 17, kind="short", form="operator", rp=20), cert_case(257, 65, kind="short", form="operator", rp=70)])
# a complement smaller than the steps: 8 directions left, the hidden 7 among them
SMALL_COMPLEMENT = dict(cert_case(72, 64, kind="hidden7"), id="packed-n72-npos64-m10-hidden7")
# npos_in + steps + 1 > cap = 42
TOO_SMALL = dict(cert_case(130, 32), ws_rank=20, id="packed-n130-npos32-m10-cap42")


def cert_inputs(cs):
    """(A, block, normA, Z, vals): the matrix (dense, or an Operator), what the binding takes for it (dict(packed=) or
    dict(operator=)), |A|_2, the locked pairs"""
    n, npos = cs["n"], cs["npos"]
    if cs["form"] == "packed":
        hidden = dict(clean=(), hidden7=(7.0,), hidden555=(5.0, 5.0, 5.0), short=())[cs["kind"]]
        A, packed, normA, Q, ev = spectrum(n, npos + (1 if cs["kind"] == "short" else 0), hidden=hidden)
        return A, dict(packed=packed), normA, Q[:, :npos], ev[:npos]
    pos = npos + (1 if cs["kind"] == "short" else 0)
    support, values, F, lam, normA, w, U = operator_pieces(n, pos, cs["rp"])
    A = O.Operator(n, support, values, F, lam)
    return A, dict(operator=dict(support=support, values=values, F=F, lam=lam)), normA, U[:, :npos], w[:npos]


def decision(theta, scale, posres=POSRES):
    """the caller's test of a certificate (full_eig_by_lanczos): True = nothing positive is left"""
    return bool(theta <= posres * scale)


def cert_scale(theta, d0, vals):
    return max(abs(d0), abs(theta), abs(vals[0]) if len(vals) else 0.0)


# ------------------------------------------------------------------------------------------------ the hazard of e
@functools.lru_cache(maxsize=1)
def hazard():
    """test_lanczos_served_full_eig_is_certified_on_every_call's exact hazard: a diagonal matrix with 7 and a triple 5, a start
    vector with zeros at the coordinates of 7 and of two copies of 5.  Returns (A, packed, lam, deficient start, nev = 4)."""
    n = 257
    rng = np.random.default_rng(11)
    lam = -rng.uniform(0.5, 3.0, n)
    top = [9.0, 7.0, 5.0, 5.0, 5.0, 3.0, 1.0]
    lam[:len(top)] = top
    A = np.diag(lam)
    deficient = rng.standard_normal(n)
    deficient[[1, 3, 4]] = 0.0
    return A, svec(A), lam, deficient, len(top) - 3
