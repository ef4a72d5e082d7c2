"""Cases, checks and the plain reference of the per-cycle tests of the Lanczos engine (test_lanczos_cycles.py on the GPU,
test_lanczos_cycles_host.py on the CPU).

A cycle of the thick-restart run leaves a basis V[:, 0..K], the coefficients alpha_k, beta_k of its own steps k >= kfirst and
-- after a restart -- the arrow part D, f of its kept columns.  Whatever order the kernels add in and whichever part of the
Gram-Schmidt passes they predict, these must form a Krylov-Schur decomposition

    A V[:, :K] = V[:, :K+1] Tbar,   T = [diag(D) f; f' tridiag(alpha, beta)],   Tbar = [T; beta_{K-1} e_K']

with V orthonormal and the coefficients the Rayleigh quotients of their columns.  `quantities` measures that in long double;
`reference_cycle` is the textbook fp64 form (two measured classical Gram-Schmidt passes per step) whose own values, for the
same inputs, are the yardstick: bound = MARGIN x max(reference, 2^-52).

Where these take a dense A they also take an OPERATOR (operator_cycle_cases.Operator: a matrix known by its pieces, so that
n > 4096 needs no dense matrix): an object with `shape`, `A @ v` in plain fp64 and `times_ld(V)` = A V in long double."""
import functools
import math

import numpy as np

from oracle import eig as oeig
from proxsdp_jl_amd.state_io import svec

LD = np.longdouble
EPS = 2.0 ** -52
MARGIN = 8.0                                       # kernel / reference, every quantity (the kernels add in tile and tree order
FLOOR = MARGIN * EPS                               # and predict the first pass); the floor where the reference is below 2^-52
HOST_BOUND = 32.0 * EPS                            # x sqrt(K): what the reference itself must stay below, so no bound is vacuous
QUANTITIES = ("r1_all", "r1_own", "r2", "r2_own", "r3_alpha", "r3_beta")
SEED = 20260
TOL = 1e-12


def case(n, nev, kd, oracle_cycles, engine, tag, flags=(), **opts):
    o = dict(eigsolver_min_lanczos=kd)
    o.update(opts)
    cycles = 3 if oracle_cycles is None or oracle_cycles >= 3 else 2
    return dict(n=n, nev=nev, kd=kd, oracle_cycles=oracle_cycles, engine=engine, opts=o, cycles=cycles, flags=tuple(flags),
                id=f"n{n}-nev{nev}-K{kd}-{tag}")


# n, nev, krylovdim, cycles the oracle needs at tol 1e-12, the engine lz_plan must choose, settings.  flags: what at least one
# captured cycle must report.  Speculation: the step and wide engines speculate the first mat-vec of cycle 3 (cycle 2 ran a
# restart); the one-workgroup kernel never does.
CASES = [
    # one row block / a last row block of one row
    case(64, 3, 12, 5, "step", "step", ("speculated",), lanczos_cycle_kernel=0),
    case(64, 3, 12, 5, "block1", "block1", lanczos_cycle_kernel=2),
    case(65, 6, 13, 11, "step", "step", ("speculated",), lanczos_cycle_kernel=0),
    case(65, 6, 13, 11, "block1", "block1", lanczos_cycle_kernel=2),
    # the one-workgroup kernel's largest K region (B1_KMAX = 31); host_eig_merge = 1 splits from krylovdim 24 on, which keeps
    # the step kernels in charge (block1_plan) and merges on the host (the device merge starts at 64 columns)
    case(129, 14, 30, 4, "step", "step", ("speculated",), lanczos_cycle_kernel=0),
    case(129, 14, 30, 4, "block1", "block1", lanczos_cycle_kernel=2),
    case(129, 14, 30, 4, "block1", "auto"),
    case(129, 14, 30, 4, "step", "merge24", ("split", "speculated"), host_eig_merge=1),
    # NCH = 2, split cycle and device merge, a side just past the one-workgroup kernel's auto range
    case(257, 34, 70, 3, "step", "step", ("split", "merge_on_device", "speculated")),
    # NCH = 3, keep in (64, 128]
    case(300, 64, 130, 3, "step", "step", ("split", "merge_on_device", "speculated")),
    # NCH = 4, keep >= 132: the jj >= 128 loop of f'h
    case(330, 109, 220, 2, "step", "step", ("split", "merge_on_device")),
    # LZ_KMAX
    case(384, 127, 255, 2, "step", "step", ("split", "merge_on_device")),
    # the wide kernels: both passes measured
    case(400, 130, 261, 2, "wide", "wide", lanczos_wide_krylov=1),
    # nt = 65, pld = 128: every "n > 4096" loop
    case(4097, 3, 8, 18, "step", "step", ("speculated",)),
    # dsaupd's acceptance and keep rule on the same engine (no split: its wanted set is re-ordered afterwards)
    case(257, 34, 70, None, "step", "arpack", ("speculated",), eigsolver=1),
]
STOP_CASES = [dict(n=130, nev=8, kd=30, rank=5, engine=e, opts=dict(eigsolver_min_lanczos=30, lanczos_cycle_kernel=k), id=f"rank5-{e}")
              for e, k in (("step", 0), ("block1", 2))]


@functools.lru_cache(maxsize=None)
def matrix(n, nev):
    """A = Q diag(ev) Q' (symmetrised), ev = linspace(12, 10, nev + 4) then n - nev - 4 values uniform in (-5, 1); |A|_2 = 12.
    Returns (A, packed, normA)."""
    rng = np.random.default_rng(SEED + 1000 * n + nev)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.concatenate([np.linspace(12.0, 10.0, nev + 4), rng.uniform(-5.0, 1.0, n - nev - 4)])
    A = (Q * ev) @ Q.T
    A = (A + A.T) / 2
    A.setflags(write=False)
    return A, svec(A), 12.0


@functools.lru_cache(maxsize=1)
def rank5_matrix(n):
    """an exact rank-5 matrix: five orthogonal +-1 / 0 vectors with disjoint supports (every product is a small integer)"""
    A = np.zeros((n, n))
    rng = np.random.default_rng(SEED + n)
    perm = rng.permutation(n)
    for q, lam in enumerate((9.0, 7.0, 5.0, 3.0, 2.0)):
        u = np.zeros(n)
        idx = perm[q * 16:(q + 1) * 16]
        u[idx] = rng.choice([-1.0, 1.0], 16) / 4.0                    # |u| = 1, entries +-1/4
        A += lam * np.outer(u, u)
    assert np.linalg.matrix_rank(A) == 5
    A.setflags(write=False)
    return A, svec(A), 9.0


def start(n):
    """the project's fixed start vector as the driver normalises it (lanczos_start_vector: the generator's vector, already of
    norm 1 up to rounding, divided by the square root of its sequentially added squares)"""
    v = oeig.start_vector(n)
    return v / np.sqrt(np.cumsum(v * v)[-1])


# ------------------------------------------------------------------------------------------------ the plain reference
def reference_cycle(A, V, kfirst, K, variant="cgs2"):
    """K - kfirst Lanczos steps in plain fp64 from V[:, :kfirst + 1]: w = A v_k, two measured classical Gram-Schmidt passes
    against V[:, :k + 1], alpha_k = the two passes' coefficients along v_k, beta_k = |w|, v_{k+1} = w / beta_k.  Returns
    (V, alphas, betas) with the coefficients at their step's index.
    Deliberately wrong variants (the host test shows that the checks tell them apart): "one_pass" = the second pass left out;
    "no_fh" = the first pass predicted from the recurrence WITHOUT the f'h row of the arrow (the kept columns are cleaned by
    nothing) and the second measured against v_{k-1}, v_k only; "alpha_1e13" = alpha_k off by 1e-13 |alpha_k|."""
    n = A.shape[0]
    V = np.array(V[:n, :K + 1], dtype=np.float64, order="F")
    V[:, kfirst + 1:] = 0.0
    al, be = np.zeros(K + 1), np.zeros(K + 1)
    for k in range(kfirst, K):
        w = A @ V[:, k]
        B = V[:, :k + 1]
        if variant == "no_fh":
            lo = max(k - 1, kfirst)
            h1 = np.zeros(k + 1)
            h1[lo:] = B[:, lo:].T @ w
            w = w - B @ h1
            h2 = np.zeros(k + 1)
            h2[lo:] = B[:, lo:].T @ w
            w = w - B @ h2
        else:
            h1 = B.T @ w
            w = w - B @ h1
            h2 = np.zeros(k + 1)
            if variant != "one_pass":
                h2 = B.T @ w
                w = w - B @ h2
        al[k] = h1[k] + h2[k]
        if variant == "alpha_1e13":
            al[k] *= 1.0 + 1e-13
        be[k] = np.linalg.norm(w)
        if be[k] == 0.0:
            break
        V[:, k + 1] = w / be[k]
    return V, al, be


def restart(V, K, kfirst, D, f, al, be, nev, kd, tol, arpack=False):
    """the Krylov-Schur restart in NumPy (KrylovKit's keep rule, or dsaupd's as the library restates it).  Returns
    (converged, done, keep, Vnext, Dkeep, fkeep)."""
    T = tmatrix(K, kfirst, D, f, al, be, np.float64)[:K, :K]
    Dasc, Uasc = np.linalg.eigh(T)
    Dd, U = Dasc[::-1], Uasc[:, ::-1]
    ff = be[K - 1] * U[K - 1, :]
    if arpack:
        eps23 = (EPS / 2.0) ** (2.0 / 3.0)
        conv = int(sum(abs(ff[i]) <= tol * max(eps23, abs(Dd[i])) for i in range(min(nev, K))))
        keep = min(kd - 1, nev + max(1, (kd - nev) // 2))
    else:
        conv = 0
        while conv < K and abs(ff[conv]) <= tol:
            conv += 1
        keep = (3 * kd + 2 * conv) // 5
    Vn = np.zeros_like(V)
    Vn[:, :keep] = V[:, :K] @ U[:, :keep]
    Vn[:, keep] = V[:, K]
    return conv, conv >= nev, keep, Vn, Dd[:keep].copy(), ff[:keep].copy()


def reference_run(A, v0, nev, kd, cycles, tol=TOL, arpack=False, variant="cgs2"):
    """`cycles` cycles of the reference with the restart above between them: a list of cycle dicts shaped as the binding's
    (kfirst, K, V, alphas, betas, D, f), and whether the run had converged before the last of them."""
    n = A.shape[0]
    V = np.zeros((n, kd + 1))
    V[:, 0] = v0 / np.linalg.norm(v0)
    kfirst, D, f = 0, np.zeros(0), np.zeros(0)
    out, early = [], False
    for c in range(cycles):
        V, al, be = reference_cycle(A, V, kfirst, kd, variant)
        out.append(dict(kfirst=kfirst, K=kd, V=V.copy(), alphas=al, betas=be, D=D, f=f))
        if c + 1 == cycles:
            break
        conv, done, keep, V, D, f = restart(V, kd, kfirst, D, f, al, be, nev, kd, tol, arpack)
        early = early or done
        kfirst = keep
    return out, early


# ------------------------------------------------------------------------------------------------ the checks, in long double
def tmatrix(K, kfirst, D, f, al, be, dtype=LD):
    """Tbar, (K + 1) x K: the arrow block (D, f), the tridiagonal of the cycle's own steps, beta_{K-1} below it"""
    T = np.zeros((K + 1, K), dtype=dtype)
    for j in range(kfirst):
        T[j, j] = D[j]
        if kfirst < K:
            T[j, kfirst] = f[j]
        T[kfirst, j] = f[j]
    for k in range(kfirst, K):
        T[k, k] = al[k]
        T[k + 1, k] = be[k]
        if k + 1 < K:
            T[k, k + 1] = be[k]
    return T


def times_a(A, V, reuse=None, chunk=512):
    """A V in long double, by row chunks of A (n = 4097: 16 n^2 bytes at once is a quarter of a gigabyte).  reuse = (V', A V'):
    columns of V that are bit-equal to the same column of V' take theirs."""
    n, K = V.shape
    out = np.zeros((n, K), dtype=LD)
    todo = list(range(K))
    if reuse is not None:
        Vo, AVo = reuse
        same = [j for j in range(min(K, Vo.shape[1], AVo.shape[1])) if np.array_equal(V[:, j], Vo[:, j])]
        out[:, same] = AVo[:, same]
        todo = [j for j in range(K) if j not in set(same)]
    if todo and hasattr(A, "times_ld"):
        out[:, todo] = A.times_ld(V[:, todo])
    elif todo:
        Vl = V[:, todo].astype(LD)
        for r0 in range(0, n, chunk):
            out[r0:r0 + chunk, todo] = A[r0:r0 + chunk].astype(LD) @ Vl
    return out


def quantities(A, normA, cyc, reuse=None):
    """R1 - R3 of one cycle (a dict with kfirst, K, V, alphas, betas, D, f; V has at least n rows and K + 1 columns), every
    product in long double.  Returns (dict of the QUANTITIES and beta_min, (V[:, :K], A V[:, :K]) for a later `reuse`)."""
    assert np.finfo(LD).eps < 1e-18
    n = A.shape[0]
    K, kf = cyc["K"], cyc["kfirst"]
    V = np.asarray(cyc["V"])[:n, :K + 1]
    Vl = V.astype(LD)
    AV = times_a(A, V[:, :K], reuse)
    T = tmatrix(K, kf, cyc["D"], cyc["f"], cyc["alphas"], cyc["betas"])
    R = np.abs(AV - Vl @ T) / LD(normA)
    G = np.abs(Vl.T @ Vl - np.eye(K + 1, dtype=LD))
    own = np.arange(kf, K)
    ra = np.einsum("ij,ij->j", Vl[:, own], AV[:, own])
    rb = np.einsum("ij,ij->j", Vl[:, own + 1], AV[:, own])
    al = np.asarray(cyc["alphas"])[own].astype(LD)
    be = np.asarray(cyc["betas"])[own].astype(LD)
    # (after a restart r1_all and r2 are mostly the kept columns', which the restart rotation left and the cycle only read:
    # r1_own and r2_own -- the cycle's new columns k > kfirst against all columns -- are the cycle's own work)
    q = dict(r1_all=float(R.max()), r1_own=float(R[:, kf:].max()), r2=float(G.max()), r2_own=float(G[:, kf + 1:].max()),
             r3_alpha=float(np.abs(al - ra).max() / LD(normA)), r3_beta=float(np.abs(be - rb).max() / LD(normA)),
             beta_min=float(be.min()))
    return q, (V[:, :K], AV)


def bound(ref_value):
    return MARGIN * max(ref_value, EPS)


def span_residual(Vprev, Kprev, Vkept):
    """max |v - P v| over the kept columns, P the projector on span(Vprev[:, :Kprev]) -- two long double Gram-Schmidt passes
    (the previous basis is orthonormal to the R2 bound only)"""
    B = Vprev[:, :Kprev].astype(LD)
    R = Vkept.astype(LD)
    for _ in range(2):
        R = R - B @ (B.T @ R)
    return float(np.abs(R).max())


def ratio_lines(cid, c, cyc, qk, qr):
    """one line of profiles/lanczos_cycles.md per cycle"""
    paths = cyc["engine"] + ("+split" if cyc["split"] else "") + ("+devmerge" if cyc["merge_on_device"] else "") + \
        ("+spec" if cyc["speculated"] else "")
    cells = " | ".join(f"{qk[q]:.2e} / {qr[q]:.2e} = {qk[q] / max(qr[q], EPS):.2f}" for q in QUANTITIES)
    return f"| {cid} | {c + 1} | {cyc['kfirst']} | {cyc['K']} | {paths} | {cells} |"
