"""Shared by the warm-start tests (host and GPU): the NumPy / SciPy restatement of the start path of
proxsdp_hip_solve_from (include/proxsdp_hip.h proxsdp_start) -- a point in the units of a result brought into the solver's
order and scale, M x and M'y of it -- and the oracle state such a start corresponds to."""
import copy

import numpy as np
import scipy.sparse as sp

import oracle
from oracle import api as oapi
from oracle import pdhg as opdhg


def psd_sides(pr):
    return [int(round((np.sqrt(8.0 * len(v) + 1.0) - 1.0) / 2.0)) for v in pr.psd]


def svec(X):
    """packed upper triangle, column by column, off-diagonals x sqrt(2): the solver's form of a PSD block"""
    n = X.shape[0]
    jj = np.repeat(np.arange(n), np.arange(1, n + 1))
    ii = np.concatenate([np.arange(j + 1) for j in range(n)]) if n else np.zeros(0, int)
    return np.where(ii == jj, X[ii, jj], X[ii, jj] * np.sqrt(2.0))


def triangle(X):
    """packed upper triangle with plain entries: what a result's primal holds for a PSD cone"""
    n = X.shape[0]
    jj = np.repeat(np.arange(n), np.arange(1, n + 1))
    ii = np.concatenate([np.arange(j + 1) for j in range(n)]) if n else np.zeros(0, int)
    return X[ii, jj]


class Internal:
    """The solver's view of a problem: variable order, off-diagonal mask, block offsets, M = [A;G] reordered and
    scaled (E M D when E, D are given, then sqrt(2)/2 on off-diagonal PSD columns), the cold primal step 1 / ||M||_F."""

    def __init__(self, pr, E=None, D=None):
        aff, cones = oapi.to_standard_form(pr)
        A = sp.csc_matrix(np.asarray(pr.M_dense)) if getattr(pr, "M_dense", None) is not None else aff.A
        aff = opdhg.AffineSets(aff.n, aff.p, aff.m, sp.csc_matrix(A, dtype=float).copy(), sp.csc_matrix(aff.G, dtype=float).copy(),
                               np.array(aff.b, float), np.array(aff.h, float), np.array(aff.c, float))
        _, var_ordering = opdhg.preprocess(aff, cones)
        self.ord = np.argsort(var_ordering, kind="stable")
        self.n, self.p, self.m = aff.n, aff.p, aff.m
        self.E = None if E is None else np.asarray(E, float)
        self.D = None if D is None else np.asarray(D, float)
        if E is not None:
            M0 = sp.vstack([aff.A, aff.G], format="csc")
            Ms = sp.csc_matrix(sp.diags(self.E) @ M0 @ sp.diags(self.D))
            aff.A, aff.G = sp.csc_matrix(Ms[:aff.p, :]), sp.csc_matrix(Ms[aff.p:, :])
            aff.c = self.D * aff.c
        opdhg.norm_scaling(aff, cones)
        self.c = aff.c
        self.M = sp.vstack([aff.A, aff.G], format="csr")
        self.offdiag = opdhg._offdiag_mask(cones, aff.n)
        self.sides = [s.sq_side for s in cones.sdpcone]
        self.off = np.concatenate([[0], np.cumsum([s * (s + 1) // 2 for s in self.sides])]).astype(int)
        fro = float(np.sqrt(np.sum(self.M.data ** 2)))
        self.cold_step = 1.0 / (fro if fro >= 1e-10 else 1.0)

    def point(self, primal=None, dual_eq=None, dual_in=None, factors=None, cold_x=None):
        """(x, y, Mx, Mty) of a start.  cold_x: the solver's cold x (entries no start value covers)."""
        x = np.zeros(self.n) if cold_x is None else np.array(cold_x, float)
        if primal is not None:
            x = np.asarray(primal, float)[self.ord]
            x = np.where(self.offdiag, x * np.sqrt(2.0), x)
            if self.D is not None:
                x = x / self.D
        blocks = {}
        for k, f in enumerate(factors or []):
            if f is None:
                continue
            lam, V = np.asarray(f[0], float), np.asarray(f[1], float).reshape(self.sides[k], -1)
            if self.D is not None:
                lam = lam / self.D[self.off[k]]
            X = (V * lam) @ V.T
            blocks[k] = X
            x[self.off[k]:self.off[k + 1]] = svec(X)
        y = np.concatenate([np.zeros(self.p) if dual_eq is None else np.asarray(dual_eq, float),
                            np.zeros(self.m) if dual_in is None else np.asarray(dual_in, float)])
        if self.E is not None:
            y = y / self.E
        return x, y, self.M @ x, self.M.T @ y, blocks


def rule_target_rank(sides, ranks, explicit=None, initial=2):
    """target rank of every cone as proxsdp_hip_solve_from derives it (ranks[k] = -1 / None: no factors)"""
    out = []
    for k, sd in enumerate(sides):
        r = -1 if ranks is None or ranks[k] is None else int(ranks[k])
        if explicit is not None and explicit[k] > 0:
            out.append(min(int(explicit[k]), sd))
        elif r >= 0:
            out.append(min(sd, max(initial, r + 1)))
        else:
            out.append(min(max(initial, 1), sd))
    return np.array(out, dtype=np.int64)


def oracle_state0(x, y, Mx, Mty, target_rank, opt, primal_step):
    """the oracle's resume state of a start: iteration 0, zero history, cold scalars"""
    nb = len(target_rank)
    return dict(iteration=0, x=np.array(x, float), y=np.array(y, float), Mty=np.array(Mty, float), Mx=np.array(Mx, float),
                target_rank=np.array(target_rank, np.int64), current_rank=2 * np.ones(nb, np.int64), min_eig=np.zeros(nb),
                hist=np.zeros((len(opdhg.STATE_HIST), 2 * opt.convergence_window)), rank_update=0, update_cont=0, ada_count=0,
                primal_step=float(primal_step), primal_step_old=float(primal_step), dual_step=float(primal_step),
                beta=float(opt.initial_beta), theta=float(opt.initial_theta), adapt_level=float(opt.initial_adapt_level))


def oracle_warm(pr, res, target_rank, opt=None, factors=None, trace=False):
    """the oracle resumed at iteration 0 from a result in user units (its primal, or factors per cone, and duals)"""
    opt = opt or oracle.Options()
    I = Internal(pr)
    x, y, Mx, Mty, _ = I.point(res.primal, res.dual_eq, res.dual_in, factors)
    st = oracle_state0(x, y, Mx, Mty, target_rank, opt, I.cold_step)
    return oracle.solve(pr, copy.deepcopy(opt), resume=st, trace=trace)


def multi_block(seed=0, sides=(1, 2, 3, 33, 64, 65), soc_len=4, nfree=3, p=30, m=12, density=0.08, diag_c=False):
    """Random feasible model with PSD blocks of the given sides, an SOC cone (soc_len = 0: none), free variables, equality
    and inequality rows, the variables deliberately NOT in solver order (kat_problems.mixed_cones with the SOC optional and
    the row density a parameter).  diag_c: the objective only on the diagonal entries of the blocks, so that with a small
    density the support {columns with an entry or c != 0} is a strict subset of the variables."""
    from proxsdp_jl_amd.problems import Problem
    rng = np.random.default_rng(seed)
    lens = [s_ * (s_ + 1) // 2 for s_ in sides]
    n = sum(lens) + soc_len + nfree
    perm = rng.permutation(n)
    psd, pos = [], 0
    for L in lens:
        psd.append(perm[pos:pos + L].astype(np.int64)); pos += L
    soc = [perm[pos:pos + soc_len].astype(np.int64)] if soc_len else []
    pos += soc_len
    free = perm[pos:]
    x0, c = np.zeros(n), np.zeros(n)
    for s_, idx in zip(sides, psd):
        Gm = rng.standard_normal((s_, s_ + 2))
        X = Gm @ Gm.T / (s_ + 2) + 0.5 * np.eye(s_)
        W = rng.standard_normal((s_, s_)); W = W @ W.T / s_ + np.eye(s_)
        x0[idx] = triangle(X)
        cw = np.where(np.eye(s_, dtype=bool), W, 0.0 if diag_c else 2.0 * W)
        c[idx] = triangle(cw)
    if soc_len:
        u = rng.standard_normal(soc_len - 1)
        x0[soc[0][0]] = np.linalg.norm(u) + 1.0
        x0[soc[0][1:]] = u
        c[soc[0][0]] = 1.5
    x0[free] = rng.standard_normal(nfree)
    A = sp.random(p, n, density=density, random_state=rng, format="csc")
    pins = sp.csc_matrix((np.ones(nfree), (np.arange(nfree), free)), shape=(nfree, n))
    A = sp.vstack([A, pins]).tocsc()
    G = sp.random(m, n, density=density, random_state=rng, format="csc")
    return Problem(n=n, A=A, b=A @ x0, G=G, h=G @ x0 + rng.uniform(0.1, 1.0, m), c=c, psd=psd, soc=soc,
                   name=f"multi-block-s{seed}")


def random_factors(pr, ranks, seed=0):
    """factors[k] = (values, vectors) with ranks[k] columns (None: no factors): values > 0 in no particular order, vectors
    NOT orthonormal"""
    rng = np.random.default_rng(seed)
    out = []
    for sd, r in zip(psd_sides(pr), ranks):
        out.append(None if r is None else (rng.uniform(0.2, 3.0, r), rng.standard_normal((sd, r)) / np.sqrt(sd)))
    return out
